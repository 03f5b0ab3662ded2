"""GPU tier (-m gpu): every device-resident output at EXACTLY the capacity the contract asks for, inside poisoned memory.

The write-outs of sjgpu_device.h (emit_indices, emit_span, emit_bytes), the string stream's drain and the tape kernels store 16-byte vectors with scalar heads
and tails into the caller's arrays; the contract is tight (idx_words >= n + 3, tok_bytes >= idx_words, dst of len bytes, tape_cap_words, string_buf_bytes).
Here every output is a slice of a larger tensor filled with 0x5A, 4 KiB of it in front and behind, and the poison is compared on the device after every
call: a store one vector past the end shows as changed poison (never as a fault: the guards are allocated memory).  The input lies 16-byte aligned inside a
larger tensor too, followed by 4 KiB of hostile bytes -- backslashes and quotes, then 0xFF and 0x00 -- and the result must be the oracle's both times.

Expected values come from the oracle (oracle/sj_oracle.c, pinned against the reference on the CPU tier) or the live reference's dom::parser::parse where its
library travelled along -- never from a run of the library under test.  Every case asserts the road it took (profile_kernel() / last_pipeline()) and prints it.

Documents: three bodies -- sparse (NDJSON-like, long strings: emit_span<.., 4>), medium (the pair and per-chunk paths) and dense (bracket runs and digit
arrays at one offset per byte: the block expansion of emit_indices) -- at ~40 KiB, at 1 MiB + ~20 KiB (crosses a resolve group, 16 KiB segments, 4 KiB chunks)
and at 8 MiB + ~132 KiB (the large-input kernels: 128 KiB and 64 KiB tiles), each extended by 0 ... 17 commas (stage 1: n + 3 passes every residue mod 4, len
every residue mod 16) or digits (minify: out_len passes every residue mod 16), and once by an unclosed string."""
import ctypes
import os

import numpy as np
import pytest

import checkers
import jsongen
from simdjson_amd import build, capi

pytestmark = pytest.mark.gpu

GUARD = 4096
POISON = 0x5A
POISON32 = 0x5A5A5A5A
E_OVERFLOW = -5
SMALL, MID, BIG = 40 << 10, (1 << 20) + (20 << 10), (8 << 20) + (132 << 10)
RANGE = 1 << 20
TAILS = 18  # 0 ... 17 bytes behind the body

SPLIT_S1 = "k_stage1_summarize+k_resolve_groups+k_resolve_segments+k_stage1_emit"
SPLIT_TOK = "k_stage1_summarize<tokens>+k_resolve_groups+k_resolve_segments+k_stage1_emit<tokens>"
SPLIT_MIN = "k_minify_summarize+k_resolve_groups+k_resolve_segments+k_minify_emit"
# road -> (pipeline, size classes, kernel of stage 1, of stage 1 with tokens, of minify)
ROADS = {
    "split": ("split", (SMALL, MID), SPLIT_S1, SPLIT_TOK, SPLIT_MIN),
    "fused": ("fused", (SMALL, MID), "k_fused<0> (16 KiB tiles)", "k_fused<0, tokens> (16 KiB tiles)", "k_fused<1> (16 KiB tiles)"),
    "large": ("fused", (BIG,), "k_fused_pipelined<0> (8 waves, 128 KiB tiles)", "k_fused_pipelined<0, tokens> (8 waves, 128 KiB tiles)", "k_minify_onchip<8>"),
}
KINDS = ("sparse", "medium", "dense")


# ---- contexts, checkers ------------------------------------------------------------------------------------------------------------------------
def _parser(pipeline, capacity=16 << 20, small_docs="0"):
    """a context whose small documents take the tile pipelines too (SJGPU_SMALL_DOCS=0; the switch is read when the context is made)"""
    old = os.environ.get("SJGPU_SMALL_DOCS")
    os.environ["SJGPU_SMALL_DOCS"] = small_docs
    try:
        p = capi.DomParserImplementation(capacity)
    finally:
        if old is None:
            del os.environ["SJGPU_SMALL_DOCS"]
        else:
            os.environ["SJGPU_SMALL_DOCS"] = old
    p.set_pipeline(pipeline)
    return p


@pytest.fixture(scope="module")
def parsers():
    build.build_sjgpu()
    made = {}

    def get(pipeline):
        if pipeline not in made:
            made[pipeline] = _parser(pipeline)
        return made[pipeline]
    yield get
    for p in made.values():
        p.close()


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


@pytest.fixture(scope="module")
def want_parse(orc):
    """the live reference's dom::parser::parse where its library travelled along, else the oracle's (pinned against it on the CPU tier)"""
    if checkers.have_reference_lib():
        ref = checkers.Reference()
        impl = ref.best_impl()
        if impl:
            return lambda d, md=1024: ref.dom_parse(impl, d, md)
    return lambda d, md=1024: orc.dom_parse(d, md)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- guarded memory ----------------------------------------------------------------------------------------------------------------------------
class Out:
    """an output array of exactly `count` elements of `itemsize` bytes inside a tensor of poison: 4 KiB of it in front, 4 KiB and more behind.  The array
    starts 16-byte aligned (phase 0) or, for the tape, 8 bytes behind a 16-byte boundary (phase 8: the contract asks for 8-byte alignment only)."""

    def __init__(self, count, itemsize, phase=0):
        import torch
        self.nbytes = int(count) * itemsize
        self.raw = torch.full((GUARD + self.nbytes + GUARD + 32,), POISON, dtype=torch.uint8, device="cuda")
        self.at = GUARD + (-(self.raw.data_ptr() + GUARD)) % 16 + phase
        self.ptr = self.raw.data_ptr() + self.at
        assert self.ptr % 16 == phase

    def view(self, dtype):
        return self.raw[self.at: self.at + self.nbytes].view(dtype)

    def poison_again(self):
        self.raw.fill_(POISON)

    def intact_around(self, used_bytes=None):
        """nothing in front of the array, nothing from `used_bytes` on (default: behind the array) -- compared on the device"""
        used = self.nbytes if used_bytes is None else int(used_bytes)
        assert 0 <= used <= self.nbytes, (used, self.nbytes)
        return bool((self.raw[: self.at] == POISON).all().item()) and bool((self.raw[self.at + used:] == POISON).all().item())


HOSTILE = (b'\\"', b"\xff\x00")


class In:
    """a document 16-byte aligned inside a larger tensor: hostile bytes in front, room for a few more bytes of document, and at least 4 KiB of hostile bytes
    behind whatever the document's length is.  set(extra, k): the document is body + extra, what follows is pattern k."""

    def __init__(self, body, room=64):
        import torch
        self.body = checkers.as_u8(body)
        host = np.empty(GUARD + len(self.body) + room + GUARD, dtype=np.uint8)
        host[:GUARD] = np.frombuffer(HOSTILE[0] * (GUARD // 2), np.uint8)
        host[GUARD: GUARD + len(self.body)] = self.body
        self.raw = torch.from_numpy(host).cuda()
        assert self.raw.data_ptr() % 16 == 0
        self.ptr = self.raw.data_ptr() + GUARD
        self.room = room
        self.pat = [torch.from_numpy(np.frombuffer(h * ((room + GUARD) // 2 + 1), np.uint8).copy()).cuda() for h in HOSTILE]
        self.set(b"", 0)

    def set(self, extra, k):
        import torch
        assert len(extra) <= self.room
        at = GUARD + len(self.body)
        if len(extra):
            self.raw[at: at + len(extra)] = torch.from_numpy(np.frombuffer(extra, np.uint8).copy()).cuda()
        rest = self.raw.numel() - at - len(extra)
        self.raw[at + len(extra):] = self.pat[k][:rest]
        self.length = len(self.body) + len(extra)

    def doc(self):
        return self.raw[GUARD: GUARD + self.length]


# ---- documents -----------------------------------------------------------------------------------------------------------------------------------
def _text(rng, n):
    """the inside of a string: letters, blanks, operators, escapes, multi-byte characters; no control character (SJGPU_F_UNESCAPED_CTRL is not raised)"""
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxy  ,:[]{}", np.uint8)
    out = bytearray(alphabet[rng.integers(0, len(alphabet), n)].tobytes())
    pieces = (b'\\"', b"\\\\", b"\\n", "é".encode(), "€".encode(), b"\\u00e9")
    for slot in range(0, n - 60, 60):  # one piece per slot of sixty bytes: they never overlap
        piece = pieces[int(rng.integers(0, len(pieces)))]
        at = slot + int(rng.integers(0, 50))
        out[at: at + len(piece)] = piece
    return bytes(out)


def _sparse(rng, size):
    """NDJSON-like, long strings: a handful of offsets per 4 KiB chunk, whole 16 KiB spans fit one emission window"""
    parts, total = [], 0
    while total < size:
        line = b'{"id":%d,"text":"%s","more":"%s"}\n' % (int(rng.integers(0, 1 << 40)), _text(rng, int(rng.integers(150, 900))), _text(rng, int(rng.integers(0, 300))))
        parts.append(line)
        total += len(line)
    return b"".join(parts)


def _medium(rng, size):
    """sections of ~0.13 offsets per byte (a 16 KiB span overflows the window, its 8 KiB pairs fit) and of ~0.3 (chunk by chunk)"""
    parts, total = [], 0
    while total < size:
        section, pairs = [], bool(rng.integers(0, 2))
        for _ in range(int(rng.integers(200, 900))):
            if pairs:
                section.append(b'{"name":"%s","value":%d},\n' % (_text(rng, int(rng.integers(20, 44))), int(rng.integers(0, 1 << 50))))
            else:
                section.append(b'{"a":%d,"bc":"%s"},' % (int(rng.integers(0, 1 << 20)), _text(rng, int(rng.integers(2, 9)))))
        parts.append(b"".join(section) + b"\n")
        total += len(parts[-1])
    return b"".join(parts)


def _dense(rng, size):
    """bracket runs and digit arrays: about one offset per byte, a 4 KiB chunk holds more than two emission windows"""
    parts, total = [], 0
    while total < size:
        k = int(rng.integers(1, 3000))
        if rng.integers(0, 2):
            parts.append(b"[" * k + b"]" * k + b",")
        else:
            parts.append(b"[" + b",".join(b"%d" % int(d) for d in rng.integers(0, 10, k)) + b"],")
        if rng.integers(0, 8) == 0:
            parts.append(b'"%s":\n' % _text(rng, int(rng.integers(0, 40))))
        total += len(parts[-1])
    return b"".join(parts) + b"\n"


_BODIES = {}


def body(kind, size):
    """seeded; every body ends outside a string, behind a newline.  The 8 MiB class is 8 MiB of the sparse body with ~132 KiB of `kind` behind it: the large
    kernels' last tiles are of that kind, and the oracle's list stays small."""
    key = (kind, size)
    if key not in _BODIES:
        rng = np.random.default_rng([KINDS.index(kind), size])
        make = {"sparse": _sparse, "medium": _medium, "dense": _dense}[kind]
        if size == BIG:
            if ("filler", BIG) not in _BODIES:
                _BODIES[("filler", BIG)] = _sparse(np.random.default_rng(99), 8 << 20)
            _BODIES[key] = _BODIES[("filler", BIG)] + make(rng, 132 << 10)
        else:
            _BODIES[key] = make(rng, size)
        assert len(_BODIES[key]) >= size and _BODIES[key].endswith(b"\n") and b"Z" not in _BODIES[key]
    return _BODIES[key]


def variants(op):
    """what is appended to a body: 0 ... 17 commas (stage 1) or digits (minify), and an unclosed string"""
    fill = b"," if op == "stage1" else b"1"
    return [fill * j for j in range(TAILS)] + [b' "unclosed, [1, 2'] + ([b'11 "unclosed'] if op == "minify" else [])


_EXPECTED = {}


def expected(orc, op, kind, size, extra):
    """the oracle's answer for body + extra, computed once per document below 2 MiB (shared by the tests), on demand above"""
    key = (op, kind, size, extra)
    if key in _EXPECTED:
        return _EXPECTED[key]
    a = np.frombuffer(body(kind, size) + extra, np.uint8)
    if op == "stage1":
        idx, flags = orc.scan(a)
        assert not flags & capi.F_UNESCAPED_CTRL  # (such a document's n is nobody's business: it is not used for an exact capacity)
        got = (np.concatenate([idx, np.array([len(a), len(a), 0], np.uint32)]), flags)
    else:
        got = orc.minify(a)
    if size < (2 << 20):
        _EXPECTED[key] = got
    return got


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def _ran(entry, road, p):
    print(f"RAN {entry} | {road} | {p.profile_kernel()}")


# ---- stage 1 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("road", list(ROADS))
def test_stage1_at_exactly_n_plus_3(parsers, orc, road, kind):
    """sjgpu_stage1_device with idx_words = n + 3: list and sentinels are the oracle's, the flags too, and the poison in front of idx and from idx + n + 3 on is
    intact -- with both hostile tails behind the document"""
    import torch
    pipeline, sizes, kernel, _, _ = ROADS[road]
    p = parsers(pipeline)
    st = _stream()
    for size in sizes:
        src = In(body(kind, size))
        for extra in variants("stage1"):
            want, wflags = expected(orc, "stage1", kind, size, extra)
            n = len(want) - 3
            want_dev = _dev(want)
            idx = Out(n + 3, 4)
            for k in range(len(HOSTILE)):
                src.set(extra, k)
                idx.poison_again()
                assert p.stage1_device(src.ptr, src.length, idx.ptr, n + 3, st) == 0
                assert p.profile_kernel() == kernel and p.last_pipeline() == pipeline, (p.profile_kernel(), p.last_pipeline())
                gn, gflags, _ = p.result(st)
                assert (gn, gflags) == (n, wflags), (road, kind, size, len(extra), k, gn, n, gflags, wflags)
                assert torch.equal(idx.view(torch.int32), want_dev), (road, kind, size, len(extra), k)
                assert idx.intact_around(), (road, kind, size, len(extra), k, "poison around idx[0 .. n + 3)")
    _ran("sjgpu_stage1_device", f"{road}, {kind}", p)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("road", list(ROADS))
def test_stage1_with_a_list_that_does_not_fit(parsers, orc, road, kind):
    """idx_words = n + 2, n, n - 1, (n / 2) | 1 and 1: rc 0, SJGPU_F_IDX_OVERFLOW, result.n the FULL count (both resolve kernels and the single-pass kernels store
    the total: a caller sizes its retry from it), nothing written at or behind idx + idx_words -- and in front of it a word is the oracle's or still poison (a
    chunk that does not fit is dropped whole)"""
    import torch
    pipeline, sizes, kernel, _, _ = ROADS[road]
    p = parsers(pipeline)
    st = _stream()
    for size in sizes:
        src = In(body(kind, size))
        for extra in variants("stage1")[:4] + variants("stage1")[TAILS:]:  # n + 3 at every residue mod 4, and the unclosed string
            want, wflags = expected(orc, "stage1", kind, size, extra)
            n = len(want) - 3
            want_dev = _dev(want)
            src.set(extra, 0)
            for words in (n + 2, n, n - 1, (n // 2) | 1, 1):
                idx = Out(words, 4)
                assert p.stage1_device(src.ptr, src.length, idx.ptr, words, st) == 0
                assert p.profile_kernel() == kernel
                gn, gflags, _ = p.result(st)
                assert gflags == (wflags | capi.F_IDX_OVERFLOW) and gn == n, (road, kind, size, len(extra), words, gn, n, gflags, wflags)
                assert idx.intact_around(), (road, kind, size, len(extra), words, "poison around idx[0 .. idx_words)")
                got = idx.view(torch.int32)
                m = min(words, n)
                assert bool(((got[:m] == want_dev[:m]) | (got[:m] == POISON32)).all().item()) and bool((got[m:] == POISON32).all().item()), (road, kind, size, len(extra), words)
    _ran("sjgpu_stage1_device, list too small", f"{road}, {kind}", p)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("road", list(ROADS))
def test_stage1_tokens_at_exactly_n_plus_3(parsers, orc, road, kind):
    """sjgpu_stage1_tokens_device with tok_bytes = idx_words = n + 3: tok[i] == buf[idx[i]] with the ORACLE's list, and poison from tok + n + 3 on (the stream
    leaves as aligned dword stores: up to three bytes behind tok[n - 1] are the stream's own) and around idx"""
    import torch
    pipeline, sizes, _, kernel, _ = ROADS[road]
    p = parsers(pipeline)
    st = _stream()
    for size in sizes:
        src = In(body(kind, size))
        for extra in variants("stage1"):
            want, wflags = expected(orc, "stage1", kind, size, extra)
            n = len(want) - 3
            want_dev = _dev(want)
            want_tok = _dev(np.frombuffer(body(kind, size) + extra, np.uint8)[want[:n]])
            idx, tok = Out(n + 3, 4), Out(n + 3, 1)
            for k in range(len(HOSTILE)):
                src.set(extra, k)
                idx.poison_again()
                tok.poison_again()
                assert p.stage1_tokens_device(src.ptr, src.length, idx.ptr, n + 3, tok.ptr, n + 3, st) == 0
                assert p.profile_kernel() == kernel and p.last_pipeline() == pipeline, (p.profile_kernel(), p.last_pipeline())
                gn, gflags, _ = p.result(st)
                assert (gn, gflags) == (n, wflags), (road, kind, size, len(extra), k, gn, n, gflags, wflags)
                assert torch.equal(idx.view(torch.int32), want_dev), (road, kind, size, len(extra), k)
                assert torch.equal(tok.view(torch.uint8)[:n], want_tok), (road, kind, size, len(extra), k)
                assert idx.intact_around() and tok.intact_around(), (road, kind, size, len(extra), k, "poison around idx / tok")
    _ran("sjgpu_stage1_tokens_device", f"{road}, {kind}", p)


# ---- minify ---------------------------------------------------------------------------------------------------------------------------------------
def _check_minify(p, st, dst, want, tag):
    import torch
    werr, wout = want
    _, gflags, out_len = p.result(st)
    assert (gflags & ~1) == 0 and bool(gflags & 1) == (werr != 0), (tag, gflags, werr)
    if werr:  # an unclosed string voids the output (out_len = 0); the array of len bytes is still all the call may touch
        assert out_len == 0, tag
        assert dst.intact_around(), (tag, "poison around dst[0 .. len)")
        return
    assert out_len == len(wout), (tag, out_len, len(wout))
    assert torch.equal(dst.view(torch.uint8)[:out_len], _dev(wout)), tag
    assert dst.intact_around(out_len), (tag, "poison in front of dst and from dst + out_len on")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("road", list(ROADS))
def test_minify_into_exactly_len_bytes(parsers, orc, road, kind):
    """sjgpu_minify_device with dst of len bytes: the bytes are the oracle's and nothing is written from dst + out_len on -- or, when the string is unclosed,
    from dst + len on"""
    pipeline, sizes, _, _, kernel = ROADS[road]
    p = parsers(pipeline)
    st = _stream()
    for size in sizes:
        src = In(body(kind, size))
        for extra in variants("minify"):
            want = expected(orc, "minify", kind, size, extra)
            for k in range(len(HOSTILE)):
                src.set(extra, k)
                dst = Out(src.length, 1)
                assert p.minify_device(src.ptr, src.length, dst.ptr, st) == 0
                assert p.profile_kernel() == kernel and p.last_pipeline() == pipeline, (p.profile_kernel(), p.last_pipeline())
                _check_minify(p, st, dst, want, (road, kind, size, len(extra), k))
    _ran("sjgpu_minify_device", f"{road}, {kind}", p)


# ---- ranges of one resident buffer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["split", "fused"])
def test_two_ranges_at_the_final_capacity(parsers, orc, pipeline):
    """sjgpu_stage1_range_device / sjgpu_minify_range_device: the 1 MiB + 20 KiB documents as two ranges, the list's capacity the FINAL n + 3, dst of len bytes;
    after the last range: the oracle's list, bytes and flags, the poison around both intact"""
    import torch
    p = parsers(pipeline)
    st = _stream()
    kernels = set()
    for kind in KINDS:
        src = In(body(kind, MID))
        for op in ("stage1", "minify"):
            for extra in variants(op):
                want = expected(orc, op, kind, MID, extra)
                src.set(extra, 1)
                L = src.length
                assert RANGE < L <= 2 * RANGE
                out = Out(len(want[0]), 4) if op == "stage1" else Out(L, 1)
                before = carry = flags = 0
                for b, e in ((0, RANGE), (RANGE, L)):
                    if op == "stage1":
                        p.stage1_range_device(src.ptr, b, e, e < L, carry, before, out.ptr, len(want[0]), st)
                        before, f, _ = p.result(st)
                    else:
                        p.minify_range_device(src.ptr, b, e, e < L, carry, before, out.ptr, st)
                        _, f, before = p.result(st)
                    assert p.last_pipeline() == pipeline
                    kernels.add(p.profile_kernel())
                    assert f & (capi.F_INTERNAL | capi.F_IDX_OVERFLOW) == 0, (kind, op, len(extra), f)
                    flags |= f & ~(1 | capi.F_RANGE_CARRY)
                    carry = f & (1 | capi.F_RANGE_CARRY)
                tag = (pipeline, kind, op, len(extra))
                if op == "stage1":
                    assert (before, flags | (carry & 1)) == (len(want[0]) - 3, want[1]), tag
                    assert torch.equal(out.view(torch.int32), _dev(want[0])), tag
                    assert out.intact_around(), (tag, "poison around idx")
                else:  # (a range is a shard: its output is kept when the string stays open -- the CALLER voids the document's)
                    assert flags == 0 and bool(carry & 1) == (want[0] != 0), tag
                    if want[0] == 0:
                        assert before == len(want[1]) and torch.equal(out.view(torch.uint8)[:before], _dev(want[1])), tag
                    assert before <= L and out.intact_around(before), (tag, "poison around dst")
    for name in sorted(kernels):
        print(f"RAN sjgpu_stage1_range_device / sjgpu_minify_range_device | {pipeline} | {name}")


# ---- shards of one document ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pipeline", ["split", "fused"])
def test_shards_that_begin_inside_and_outside_a_string(parsers, orc, pipeline, kind):
    """sjgpu_stage1_shard_device / sjgpu_minify_shard_device at exact capacities, in_string 0 and 1.  A shard that begins inside a string is the rest of a
    document whose first sixteen bytes -- `["xxxxxxxxxxxxxx` -- lie in front of it: the oracle scans that document, the shard's list is what lies behind byte 16"""
    import torch
    p = parsers(pipeline)
    st = _stream()
    head = b'["' + b"x" * 14
    kernels = set()
    if True:
        for size in (SMALL, MID):
            for in_string in (0, 1):
                lead = b'yz in a string", 1, 2]\n' if in_string else b""
                src = In(lead + body(kind, size))
                for extra in variants("stage1")[:TAILS]:
                    src.set(extra, in_string)
                    shard = lead + body(kind, size) + extra
                    L = len(shard)
                    a = np.frombuffer(head + shard if in_string else shard, np.uint8)
                    cut = len(head) if in_string else 0
                    widx, wflags = orc.scan(a) if in_string else (expected(orc, "stage1", kind, size, extra)[0][:-3], 0)
                    assert wflags == 0
                    want = np.concatenate([widx[widx >= cut] - cut, np.array([L, L, 0], np.uint32)]).astype(np.uint32)
                    n = len(want) - 3
                    idx = Out(n + 3, 4)
                    p.stage1_shard_device(src.ptr, L, in_string, idx.ptr, n + 3, st)
                    kernels.add(p.profile_kernel())
                    assert p.last_pipeline() == pipeline
                    gn, gflags, _ = p.result(st)
                    tag = (pipeline, kind, size, in_string, len(extra))
                    assert (gn, gflags) == (n, 0), (tag, gn, n, gflags)
                    assert torch.equal(idx.view(torch.int32), _dev(want)), tag
                    assert idx.intact_around(), (tag, "poison around idx")
                    # minify: digits behind the body instead of commas (out_len at every residue)
                    extra_m = b"1" * len(extra)
                    src.set(extra_m, in_string)
                    shard = lead + body(kind, size) + extra_m
                    werr, wout = orc.minify(np.frombuffer(head + shard, np.uint8)) if in_string else expected(orc, "minify", kind, size, extra_m)
                    assert werr == 0
                    wout = wout[cut:]  # (the sixteen bytes in front of the shard are all kept)
                    dst = Out(L, 1)
                    p.minify_shard_device(src.ptr, L, in_string, dst.ptr, st)
                    kernels.add(p.profile_kernel())
                    _, mflags, out_len = p.result(st)
                    assert (mflags, out_len) == (0, len(wout)), (tag, mflags, out_len, len(wout))
                    assert torch.equal(dst.view(torch.uint8)[:out_len], _dev(wout)), tag
                    assert dst.intact_around(out_len), (tag, "poison around dst")
    for name in sorted(kernels):
        print(f"RAN sjgpu_stage1_shard_device / sjgpu_minify_shard_device | {pipeline}, {kind} | {name}")


# ---- the list behind the scan: finish, depth, keys -------------------------------------------------------------------------------------------------------
def _stream_shapes():
    rng = np.random.default_rng(5)
    lines = [l for l in _sparse(rng, 60 << 10).split(b"\n") if l] + [jsongen.random_document(rng).replace(b"\n", b" ").replace(b"\r", b" ") for _ in range(200)]
    nd = b"\n".join(lines) + b"\n"
    return {"ndjson": nd, "ndjson cut inside a line": nd[:-77], "ndjson cut inside a string": nd[:-60] + b' "dangling', "rs": b"".join(b"\x1e" + l + b"\n" for l in lines),
            "rs cut": b"".join(b"\x1e" + l + b"\n" for l in lines)[:-30], "commas": b",".join(lines), "commas cut": b",".join(lines)[:-30], "commas and blanks": b" , ".join(lines) + b" ,",
            "single value": b"12345", "two scalars": b"1 2", "unbalanced": b"{[}] 1", "closers first": b']} {"a":1} [', "one document, truncated": _medium(rng, 50 << 10)[:-9]}


def test_finish_on_the_device_in_a_list_of_n_raw_plus_3(parsers, orc):
    """sjgpu_stage1_finish_device, the six streaming modes, on the list as stage 1 left it in n_raw + 3 words: what the oracle's stage1(mode) delivers (= the
    reference's finish()), equal to the library's own host path too, and nothing written behind idx + n_raw + 3"""
    import torch
    p = parsers("fused")
    host = _parser("auto", small_docs="1")
    st = _stream()
    for name, data in _stream_shapes().items():
        a = checkers.as_u8(data)
        ln = checkers.trim_partial_utf8_len(a)
        src = In(a[:ln])
        for mode in range(1, 7):
            src.set(b"", mode & 1)
            widx, wflags = orc.scan(a[:ln])
            assert not wflags & capi.F_UNESCAPED_CTRL
            n_raw = len(widx)
            idx = Out(n_raw + 3, 4)
            assert p.stage1_device(src.ptr, ln, idx.ptr, n_raw + 3, st) == 0
            assert p.result(st)[:2] == (n_raw, wflags)
            want = checkers.observable(a, mode, *orc.stage1(a, mode))
            err, n, _ = p.stage1_finish_device(src.ptr, ln, mode, idx.ptr, n_raw, wflags, st)
            got = (err,) if err in checkers.EARLY or len(want) == 1 else (err, n, tuple(int(x) & 0xFFFFFFFF for x in idx.view(torch.int32)[: n + 3].cpu().numpy()))
            assert got == want, (name, mode, got[:2], want[:2])
            assert idx.intact_around(), (name, mode, "poison around idx[0 .. n_raw + 3)")
            host.n_structural_indexes = 0  # (the oracle starts from n = 0 too: what a call leaves of a stale n is not under test here)
            herr = host.stage1(a, mode)
            hgot = checkers.observable(a, mode, herr, host.n_structural_indexes, host.structural_indexes[: host.n_structural_indexes + 3])
            assert hgot == want, (name, mode, "sjgpu_stage1 of the same bytes")
    host.close()
    print(f"RAN sjgpu_stage1_finish_device | the six streaming modes | the list of {p.profile_kernel()}")


def test_depth_scan_into_exactly_n_plus_1_words(parsers, orc):
    """sjgpu_depth_scan_device / sjgpu_depth_scan_tokens_device: depth[0 .. n] against a running count over the oracle's list, poison around the n + 1 words"""
    import torch
    p = parsers("split")
    st = _stream()
    for kind, size in (("sparse", SMALL), ("medium", MID), ("dense", SMALL), ("dense", MID)):
        for extra in (b"", b",", b",,", b",,,"):
            a = np.frombuffer(body(kind, size) + extra, np.uint8)
            want_idx, _ = expected(orc, "stage1", kind, size, extra)
            n = len(want_idx) - 3
            c = a[want_idx[:n]]
            delta = np.isin(c, [ord("{"), ord("[")]).astype(np.int64) - np.isin(c, [ord("}"), ord("]")]).astype(np.int64)
            want = _dev(np.concatenate([[0], np.cumsum(delta)]).astype(np.int32))
            src = In(a)
            idx, tok = _dev(want_idx), _dev(c)  # the oracle's own list and token bytes: the scan is the unit under test
            for tokens in (False, True):
                depth = Out(n + 1, 4)
                if tokens:
                    p.depth_scan_tokens_device(tok.data_ptr(), n, depth.ptr, st)
                else:
                    p.depth_scan_device(src.ptr, idx.data_ptr(), n, depth.ptr, st)
                torch.cuda.synchronize()
                assert torch.equal(depth.view(torch.int32), want), (kind, size, len(extra), tokens)
                assert depth.intact_around(), (kind, size, len(extra), tokens, "poison around depth[0 .. n]")
    print("RAN sjgpu_depth_scan_device / sjgpu_depth_scan_tokens_device | gathered and from the token stream | launch_depth_scan")


def test_match_keys_into_exactly_n_words(parsers, orc):
    """sjgpu_match_keys_device: one word per structural, the oracle's, and poison around the n words"""
    import torch
    p = parsers("split")
    st = _stream()
    names = [b"id", b"text", b"more", b"name", b"value", b"a", b"bc", b"", b"not_there"]
    total = 0
    for kind, size in (("sparse", SMALL), ("medium", SMALL), ("medium", MID)):
        for extra in (b"", b",", b",,", b",,,"):
            a = np.frombuffer(body(kind, size) + extra, np.uint8)
            want_idx, _ = expected(orc, "stage1", kind, size, extra)
            n = len(want_idx) - 3
            want, wm = orc.match_keys(a, want_idx[: n + 1], n, names)
            src = In(a)
            idx = _dev(want_idx)
            out = Out(n, 4)
            m = p.match_keys_device(src.ptr, len(a), idx.data_ptr(), n, names, out.ptr, st)
            assert m == wm and torch.equal(out.view(torch.int32), _dev(want)), (kind, size, len(extra), m, wm)
            assert out.intact_around(), (kind, size, len(extra), "poison around match[0 .. n)")
            total += wm
    assert total > 1000
    print("RAN sjgpu_match_keys_device | - | launch_match_keys")


# ---- strings ------------------------------------------------------------------------------------------------------------------------------------------
def _csr(noffsets, used):
    """the oracle's per-structural offsets (NO_STRING for the others) -> CSR form (offsets[i] = start of the next record, offsets[n] = bytes used)"""
    val = np.where(noffsets != checkers.NO_STRING, noffsets, np.uint32(used)).astype(np.uint32)  # (record offsets grow with i: the next record's is the minimum behind i)
    return np.concatenate([np.minimum.accumulate(val[::-1])[::-1], np.array([used], np.uint32)]).astype(np.uint32)


def _strings_call(p, src, L, idx, n, sbuf, off, st):
    used, cnt, bad = ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = p.L.sjgpu_parse_strings_device(p.h, src.ptr, L, idx.data_ptr(), n, 0, sbuf.ptr, sbuf.nbytes, off.ptr, st or None, ctypes.byref(used), ctypes.byref(cnt), ctypes.byref(bad))
    return rc, int(used.value), int(cnt.value), int(bad.value)


@pytest.mark.parametrize("walk", [False, True], ids=["stream", "walk"])
def test_strings_into_exactly_the_bytes_they_need(parsers, orc, walk, monkeypatch):
    """sjgpu_parse_strings_device on both roads (SJGPU_STRING_STREAM=0 forces the per-string walk): string_buf_bytes = the oracle's byte count, offsets of n + 1
    words: SUCCESS, the oracle's bytes and offsets, poison around both; one byte less: SJGPU_E_OVERFLOW and nothing at or behind the capacity given"""
    import torch
    p = parsers("split")
    st = _stream()
    if walk:
        monkeypatch.setenv("SJGPU_STRING_STREAM", "0")
    paths = set()
    for kind, size in (("sparse", SMALL), ("medium", SMALL), ("medium", MID), ("dense", SMALL)):
        for j in range(16):  # a last string of 0 ... 15 characters: the buffer's length at every residue mod 16
            extra = b'"' + b"s" * j + b'"'
            a = np.frombuffer(body(kind, size) + extra, np.uint8)
            want_idx, wflags = orc.scan(a)
            assert wflags == 0
            n = len(want_idx)
            werr, wbytes, woff, wstrings, wbad = orc.string_buffer(a, np.concatenate([want_idx, np.array([len(a)], np.uint32)]), n)
            assert werr == 0 and wbad == checkers.NO_STRING
            src = In(a)
            idx = _dev(np.concatenate([want_idx, np.array([len(a), len(a), 0], np.uint32)]))
            sbuf, off = Out(len(wbytes), 1), Out(n + 1, 4)
            rc, used, cnt, bad = _strings_call(p, src, len(a), idx, n, sbuf, off, st)
            tag = (kind, size, j, "walk" if walk else "stream")
            assert (rc, used, cnt, bad) == (0, len(wbytes), wstrings, checkers.NO_STRING), (tag, rc, used, cnt, bad, len(wbytes), wstrings)
            if walk or kind != "dense":  # (long stretches of brackets without a control character: the stream may decline, then the walk writes the same bytes)
                assert p.string_path() == (2 if walk else 1), (tag, p.string_path())
            paths.add(p.string_path())
            assert torch.equal(sbuf.view(torch.uint8), _dev(wbytes)), tag
            assert torch.equal(off.view(torch.int32), _dev(_csr(woff, len(wbytes)))), tag
            assert sbuf.intact_around() and off.intact_around(), (tag, "poison around the string buffer / the offsets")
            if j % 5 == 0:
                short, off2 = Out(len(wbytes) - 1, 1), Out(n + 1, 4)
                rc = _strings_call(p, src, len(a), idx, n, short, off2, st)[0]
                assert rc == E_OVERFLOW, (tag, rc)
                assert short.intact_around() and off2.intact_around(), (tag, "a call that overflows wrote behind the capacity given")
    print(f"RAN sjgpu_parse_strings_device | {'per-string walk' if walk else 'stream compaction'} | string paths {sorted(paths)}")


# ---- stage 2 ------------------------------------------------------------------------------------------------------------------------------------------
def _stage2_documents():
    """a few hundred KiB each: random documents, one nested 70 deep in the middle (the sort's second pass), one with numbers beyond 19 digits
    (k_tape_slow_numbers); then [a document with a string the reference rejects (the stream declines: road 2), its valid twin] and [a broken one, its twin]"""
    rng = np.random.default_rng(41)

    def many(count):
        return [jsongen.random_document(rng) for _ in range(count)]
    plain = b"[" + b",\n".join(many(2500)) + b"]"
    deep = b"[" + b",".join(many(900)) + b"," + b'{"d":[' * 35 + b'"bottom",1.5' + b"]}" * 35 + b"," + b",".join(many(900)) + b"]"
    longs = ["1" * 70 + ".0", "0." + "7" * 90, "1" + "0" * 200 + "e-190", "3." + "1" * 400 + "e5", "1" * 25 + "e0", "12345678901234567890.0", "0.000000000000000000000000000001e31",
             "9007199254740992.500000000000000000000000000000000001", "2.4703282292062327e-324", "1.797693134862315807e308"]
    numbers = b"[" + b",".join(many(700)) + b"," + b",".join(longs[int(k)].encode() for k in rng.integers(0, len(longs), 4000)) + b',"s"]'
    twin = b"[" + b",".join(many(1200)) + b',"x\\ny",' + b",".join(many(300)) + b"]"
    rejected = twin.replace(b'"x\\ny"', b'"x\\qy"')
    twin2 = b"[" + b",".join(many(1200)) + b',{"k":1,"l":2},' + b",".join(many(300)) + b"]"
    broken = twin2.replace(b'{"k":1,"l":2}', b'{"k":1,,"l":2}')
    return {"random": plain, "70 deep": deep, "long numbers": numbers}, {"rejected string": (rejected, twin), "broken": (broken, twin2)}


def _stage2_call(p, src, L, idx, n, tok, tape, sbuf, st):
    tw, sb = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = p.L.sjgpu_stage2_tokens_device(p.h, src.ptr, L, idx.data_ptr(), n, tok.data_ptr() if tok is not None else None, 1024, tape.ptr, tape.nbytes // 8, sbuf.ptr, sbuf.nbytes,
                                        st or None, ctypes.byref(tw), ctypes.byref(sb))
    return rc, int(tw.value), int(sb.value)


@pytest.mark.parametrize("tokens", [False, True], ids=["sjgpu_stage2_device", "sjgpu_stage2_tokens_device"])
def test_stage2_at_exactly_the_words_and_bytes_it_delivers(parsers, orc, want_parse, tokens, monkeypatch):
    """tape_cap_words = the checker's tape length (the tape slice 8-byte aligned, not 16), string_buf_bytes = its string bytes: SUCCESS, word for word, byte
    for byte, poison around both -- on both string roads; with the tape one word short and with the string buffer one byte short: SJGPU_E_OVERFLOW and nothing
    behind the capacity given.  A broken document, at the capacities of its valid twin: the checker's error code, nothing behind the capacities."""
    import torch
    p = parsers("split")
    st = _stream()
    valid, invalid = _stage2_documents()
    paths = set()

    def resident(doc):
        a = np.frombuffer(doc, np.uint8)
        widx, wflags = orc.scan(a)
        assert wflags == 0
        src = In(a)
        idx = _dev(np.concatenate([widx, np.array([len(a), len(a), 0], np.uint32)]))
        tok = _dev(a[widx]) if tokens else None
        return a, src, idx, len(widx), tok

    for name, doc in valid.items():
        a, src, idx, n, tok = resident(doc)
        werr, wtape, wstr = want_parse(a)
        assert werr == 0 and len(wstr) > 0, name
        for walk in (False, True):
            if walk:
                monkeypatch.setenv("SJGPU_STRING_STREAM", "0")
            else:
                monkeypatch.delenv("SJGPU_STRING_STREAM", raising=False)
            tape, sbuf = Out(len(wtape), 8, phase=8), Out(len(wstr), 1)
            rc, tw, sb = _stage2_call(p, src, len(a), idx, n, tok, tape, sbuf, st)
            assert (rc, tw, sb) == (0, len(wtape), len(wstr)), (name, walk, rc, tw, sb, len(wtape), len(wstr))
            assert p.string_path() == (2 if walk else 1), (name, walk)
            paths.add(p.string_path())
            assert torch.equal(tape.view(torch.int64), _dev(wtape)) and torch.equal(sbuf.view(torch.uint8), _dev(wstr)), (name, walk)
            assert tape.intact_around() and sbuf.intact_around(), (name, walk, "poison around the tape / the string buffer")
            tape, sbuf = Out(len(wtape) - 1, 8, phase=8), Out(len(wstr), 1)
            assert _stage2_call(p, src, len(a), idx, n, tok, tape, sbuf, st)[0] == E_OVERFLOW, (name, walk, "tape one word short")
            assert tape.intact_around() and sbuf.intact_around(), (name, walk, "tape one word short: poison")
            tape, sbuf = Out(len(wtape), 8, phase=8), Out(len(wstr) - 1, 1)
            assert _stage2_call(p, src, len(a), idx, n, tok, tape, sbuf, st)[0] == E_OVERFLOW, (name, walk, "string buffer one byte short")
            assert tape.intact_around() and sbuf.intact_around(), (name, walk, "string buffer one byte short: poison")
        monkeypatch.delenv("SJGPU_STRING_STREAM", raising=False)
    for name, (doc, twin) in invalid.items():
        a, src, idx, n, tok = resident(doc)
        werr = want_parse(a)[0]
        terr, ttape, tstr = want_parse(np.frombuffer(twin, np.uint8))
        assert werr != 0 and terr == 0, name
        tape, sbuf = Out(len(ttape), 8, phase=8), Out(len(tstr), 1)
        rc = _stage2_call(p, src, len(a), idx, n, tok, tape, sbuf, st)[0]
        assert rc == werr, (name, rc, werr)
        if name == "rejected string":
            assert p.string_path() == 2, name  # the stream declined, the per-string kernels found the string
        assert tape.intact_around() and sbuf.intact_around(), (name, "poison around the tape / the string buffer")
    assert paths == {1, 2}
    print(f"RAN {'sjgpu_stage2_tokens_device' if tokens else 'sjgpu_stage2_device'} | string roads 1 and 2, the sort in one and two passes | launch_tape_front + launch_parse_strings + launch_tape")


# ---- the host entry points ------------------------------------------------------------------------------------------------------------------------------
def _pinned(count, dtype, fill):
    """a page-locked numpy array with a 4 KiB guard in front and behind: (whole, inner view); release with capi.host_unregister(whole)"""
    guard = GUARD // np.dtype(dtype).itemsize
    whole = np.full(guard + count + guard, fill, dtype=dtype)
    capi.host_register(whole)
    return whole, whole[guard: guard + count], guard


def test_host_entry_points_keep_to_their_arrays(orc):
    """sjgpu_stage1 with idx_words = len + 3 (a document of at most 64 KiB: k_docs; one of 200 KiB: the kernels write the list into page-locked host memory
    and the call copies n + 3 words), sjgpu_minify with dst of exactly len bytes, sjgpu_stage1_many with three documents whose lists lie back to back: the
    oracle's results, nothing behind idx[n + 2], nothing behind dst + len, no neighbour touched"""
    p = _parser("auto", 4 << 20, small_docs="1")
    rng = np.random.default_rng(8)
    def records(size):
        parts, total = [], 0
        while total < size:
            parts.append(b'{"name":"%s","value":%d,"tags":[%d,true,null]}\n' % (_text(rng, int(rng.integers(0, 90))), int(rng.integers(0, 1 << 50)), int(rng.integers(0, 99))))
            total += len(parts[-1])
        return parts
    small, large = b"".join(records(40 << 10)), b"".join(records(200 << 10))
    assert len(small) <= (64 << 10) and len(large) > (200 << 10)
    for doc, kernel in ((small, "k_docs<0>"), (large, None)):
        a = np.frombuffer(doc, np.uint8).copy()
        L = len(a)
        werr, wn, widx = orc.stage1(a, 0)
        assert werr == 0
        whole, idx, g = _pinned(L + 3, np.uint32, POISON32)
        try:
            n, nxt = ctypes.c_uint32(0), ctypes.c_uint32(0)
            rc = p.L.sjgpu_stage1(p.h, a.ctypes.data, L, 0, idx.ctypes.data, L + 3, ctypes.byref(n), ctypes.byref(nxt))
            assert (rc, n.value) == (0, wn) and np.array_equal(idx[: wn + 3], widx), (L, rc, n.value, wn)
            if kernel:
                assert p.profile_kernel() == kernel
            print(f"RAN sjgpu_stage1 | host buffer of {L} bytes | {p.profile_kernel()}")
            assert (whole[:g] == POISON32).all() and (whole[g + wn + 3:] == POISON32).all(), (L, "poison in front of idx and behind idx[n + 2]")
        finally:
            capi.host_unregister(whole)
        merr, mout = orc.minify(a)
        whole, dst, g = _pinned(L, np.uint8, POISON)
        try:
            out_len = ctypes.c_size_t(0)
            rc = p.L.sjgpu_minify(p.h, a.ctypes.data, L, dst.ctypes.data, ctypes.byref(out_len))
            assert (rc, out_len.value) == (merr, len(mout)) and np.array_equal(dst[: len(mout)], mout), (L, rc, out_len.value)
            print(f"RAN sjgpu_minify | host buffer of {L} bytes | {p.profile_kernel()}")
            assert (whole[:g] == POISON).all() and (whole[g + L:] == POISON).all(), (L, "poison in front of dst and behind dst + len")
        finally:
            capi.host_unregister(whole)
    # three lists back to back in one array: [len0 + 3][len1 + 3][len2 + 3]; behind each list's n + 3 words the poison stays, and so does every neighbour
    docs = [np.frombuffer(d, np.uint8).copy() for d in (b"".join(records(5000)), b'{"a":[1,2,{"b":null}],"c":"d"}', b"".join(records(25001)))]
    want = [orc.stage1(d, 0) for d in docs]
    total = sum(len(d) + 3 for d in docs)
    whole, pool, g = _pinned(total, np.uint32, POISON32)
    try:
        batch = (capi.Doc * 3)()
        at, begins = 0, []
        for k, d in enumerate(docs):
            batch[k] = capi.Doc(d.ctypes.data, len(d), pool[at:].ctypes.data, len(d) + 3, 0, 0)
            begins.append(at)
            at += len(d) + 3
        assert p.L.sjgpu_stage1_many(p.h, batch, 3) == 0
        print(f"RAN sjgpu_stage1_many | three host buffers, lists back to back | {p.profile_kernel()}")
        for k, (d, (werr, wn, widx)) in enumerate(zip(docs, want)):
            assert (batch[k].error, batch[k].n) == (werr, wn), (k, batch[k].error, batch[k].n, werr, wn)
            mine = pool[begins[k]: begins[k] + len(d) + 3]
            assert np.array_equal(mine[: wn + 3], widx) and (mine[wn + 3:] == POISON32).all(), (k, "list and the poison behind idx[n + 2]")
        assert (whole[:g] == POISON32).all() and (whole[g + total:] == POISON32).all()
    finally:
        capi.host_unregister(whole)
    p.close()
