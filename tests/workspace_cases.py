"""The plan of tests/test_gpu_workspace.py: documents and call sequences that walk the single-pass workspace up and down.

A single-pass call is ONE dispatch: k_fused, k_fused_pipelined and k_minify_onchip clear nothing in front of themselves, each trusts that the kernel before
it -- whichever it was -- left [tile descriptors][control words] all zero (sjgpu_fused.hip: leave_and_clean).  The control words have no fixed address:
they lie behind THIS call's ntiles descriptors, and ntiles follows the span scanned and the kernel's tile size -- 16 KiB for k_fused, 128 KiB for the
eight-wave pipelined kernel, 64 KiB for k_minify_onchip.  So one call's [ticket, done][flags] ... [second ticket counter] are a later call's descriptors
and the other way round, and a word left behind at desc[A + k] does nothing until a call with more than A + k tiles arrives.  The sequences below put every
control-word slot of a short call under a descriptor of the next call and back, take the six kernels in turn on one context, end calls in every way a
call can end, and change road and allocation in between.  tests/test_workspace_cases.py (CPU tier) checks what this file claims about itself -- the
documents' kinds by the oracle, the tile counts and the kernels reached by the constants of sjgpu_internal.h / sjgpu_ctx.h -- so that the GPU test can be
read against a table."""
import collections
import functools

import numpy as np

import jsongen
from simdjson_amd import corpus

KIB, MIB = 1 << 10, 1 << 20
# (retyped here for the plan; tests/test_workspace_cases.py reads them out of the headers and compares)
TILE_SMALL, TILE_PIPELINED, TILE_ONCHIP = 16 * KIB, 128 * KIB, 64 * KIB  # k_fused | k_fused_pipelined (8 waves) | k_minify_onchip<8>
SMALL_BELOW = 8 * MIB        # FUSED_SMALL_BELOW: spans up to here take the 16 KiB-tile kernels
AUTO_FUSED_BELOW = 5 * MIB   # AUTO: single pass up to here; beyond it the split pipeline at every size this plan has
CTL_WORDS = 18               # FUSED_WORKSPACE_EXTRA_WORDS: [ticket, done][flags, -], fourteen words of distance, [second ticket counter]
SECOND_TICKET_WORD = 16
MAX_BYTES = 13 * MIB

F_UNCLOSED_STRING, F_UNESCAPED_CTRL, F_UTF8_ERROR, F_IDX_OVERFLOW = 1, 2, 4, 8
SUCCESS, UTF8_ERROR, UNESCAPED_CHARS, UNCLOSED_STRING = 0, 11, 14, 15

# kind -> (flags of the raw scan, error code of stage 1): what the document CLAIMS; checkers.Oracle() decides (tests/test_workspace_cases.py)
KINDS = {
    "dense": (0, SUCCESS),            # corpus.large_random
    "sparse": (0, SUCCESS),           # corpus.amazon_ndjson
    "escape_heavy": (0, SUCCESS),     # the runs of corpus.escape_heavy
    "runs": (0, SUCCESS),             # a 200-byte backslash run across every 16 KiB border: the look-back meets x words (lookback_general)
    "in_string_tail": (0, SUCCESS),   # the part of a document behind its first 16 bytes, which end inside a string (a shard with in_string = 1)
    "unclosed": (F_UNCLOSED_STRING, UNCLOSED_STRING),  # an unclosed string at the end
    "ctrl": (F_UNESCAPED_CTRL, UNESCAPED_CHARS),       # a control character inside a string, in the middle
    "bad_utf8": (F_UTF8_ERROR, UTF8_ERROR),            # a byte 0xFF inside a string, in the middle
}
VALID = ("dense", "sparse", "escape_heavy", "runs")
HEAD = b'["0123456789abcd'  # 16 bytes in front of an in_string_tail: with them it is a document again
assert len(HEAD) == 16

Doc = collections.namedtuple("Doc", "kind length seed")
# op: the entry point; pipeline: "fused" | "split" | "auto", set in front of the call; extra: a dict -- idx_words ("n+2": the list does not fit),
# in_string (shards), part / cut (ranges: part 0 is [0, cut), part 1 [cut, length)), set_capacity (in front of the call)
Call = collections.namedtuple("Call", "op pipeline doc extra")

STAGE1_OPS = ("stage1_device", "stage1_shard_device", "stage1_range_device")
TOKEN_OPS = ("stage1_tokens_device",)
MINIFY_OPS = ("minify_device", "minify_shard_device", "minify_range_device")
OTHER_OPS = ("validate_utf8_device", "string_parity_device")  # kernels of their own: they write the result and must not touch the workspace
SIX_KERNELS = ("k_fused<0>", "k_fused<0, tokens>", "k_fused<1>", "k_fused_pipelined<0>", "k_fused_pipelined<0, tokens>", "k_minify_onchip<8>")


# ---- documents: by kind, EXACT byte length and seed ---------------------------------------------------------------------------------------------
def _filler(rng, room):
    """exactly `room` bytes of small valid documents (jsongen), a newline in front of each, blanks behind the last"""
    out, misses = bytearray(), 0
    while misses < 8 and room - len(out) > 2:
        d = jsongen.random_document(rng)
        if len(out) + 1 + len(d) <= room:
            out += b"\n" + d
        else:
            misses += 1
    return bytes(out) + b" " * (room - len(out))


def _escape_runs(length, seed):
    """strings that are almost nothing but backslash runs, the run lengths of corpus.escape_heavy in its order, as many as fit"""
    rot = int(seed) % len(corpus.ESCAPE_RUNS)
    order = corpus.ESCAPE_RUNS[rot:] + corpus.ESCAPE_RUNS[:rot]
    runs, used, k, misses = [], 2, 0, 0
    while misses < len(order):
        r = order[k % len(order)]
        k += 1
        cost = r + 3 + (2 if r % 2 else 0)
        if used + cost <= length - 8:
            runs.append(r)
            used += cost
            misses = 0
        else:
            misses += 1
    return corpus.backslash_runs(runs)


def _runs(length):
    """text with a string across every 16 KiB border whose 200 backslashes lie 100 in front of the border and 100 behind: the 64 bytes in front of the
    next tile's first span do not settle the escape state, the span assumes, and an x word travels through the descriptors (sj_xcarry.h)"""
    unit, piece = b'12, "k", ', b' "' + b"a" * 50 + b"\\" * 200 + b'", '

    def text(n):
        return unit * (n // len(unit)) + b" " * (n % len(unit))
    parts, pos = [b"["], 1
    for border in range(TILE_SMALL, length - 512, TILE_SMALL):
        start = border - 152  # ` "`, fifty letters, then the run: its 101st backslash is the first byte behind the border
        parts += [text(start - pos), piece]
        pos = start + len(piece)
    parts += [text(length - pos - 4), b'"e"]']
    return np.frombuffer(b"".join(parts), np.uint8)


def _valid(kind, length, seed):
    if kind == "runs":
        return _runs(length)
    rng = np.random.default_rng([int(seed), int(length)])
    if kind == "escape_heavy":
        body = _escape_runs(length, seed)
    else:
        make = {"dense": corpus.large_random, "sparse": corpus.amazon_ndjson}[kind]
        body = make(max(length - 8192 - 64, 64), seed)[0]  # (the generators stop within 8 KiB behind their target)
    assert len(body) <= length, (kind, length, len(body))
    return np.concatenate([body, np.frombuffer(_filler(rng, length - len(body)), np.uint8)])


def _spliced(length, seed, piece):
    """a valid document, `piece`, another valid document: `length` bytes"""
    front = (length - len(piece)) // 2
    return np.concatenate([_valid("dense", front, seed), np.frombuffer(piece, np.uint8), _valid("sparse", length - len(piece) - front, seed + 1)])


@functools.lru_cache(maxsize=None)
def make(doc):
    """the document's bytes: a read-only uint8 array of exactly doc.length bytes"""
    kind, length, seed = doc
    assert 4096 <= length <= MAX_BYTES and kind in KINDS
    if kind in VALID:
        a = _valid(kind, length, seed)
    elif kind == "in_string_tail":
        lead = b' still inside the string", '
        a = np.concatenate([np.frombuffer(lead, np.uint8), _valid("dense", length - len(lead), seed)])
    elif kind == "unclosed":
        tail = b' "dangling text'
        a = np.concatenate([_valid("sparse", length - len(tail), seed), np.frombuffer(tail, np.uint8)])
    elif kind == "ctrl":
        a = _spliced(length, seed, b'\n["a control character \x01 inside a string"]\n')
    else:
        a = _spliced(length, seed, b'\n["not UTF-8: \xff"]\n')
    a = np.ascontiguousarray(a, np.uint8)
    assert len(a) == length, (doc, len(a))
    a.setflags(write=False)
    return a


def oracle_input(doc):
    """what the oracle is asked about: the document -- for an in_string_tail, the document with its head"""
    return np.concatenate([np.frombuffer(HEAD, np.uint8), make(doc)]) if doc.kind == "in_string_tail" else make(doc)


# ---- lengths, by tile count ---------------------------------------------------------------------------------------------------------------------
BORDER_TILES = (1, 2, 3, 17, 18, 19, 64)
SMALL_LENGTHS = tuple(t * TILE_SMALL + d for t in BORDER_TILES for d in (-1, 0, 1))
# the 128 KiB- and 64 KiB-tile kernels are reached above 8 MiB only.  12 MiB + 17: 97 tiles of 128 KiB (odd), 193 of 64 KiB (odd); 8 MiB + 128 KiB: 65 and 130;
# 8 MiB + 1: 65 and 129; 9 MiB - 1: 72 and 144 -- an even and an odd tile count for either size, and so for the even / odd ticket streams of minify
BIG_1, BIG_EXACT, BIG_9, BIG_12 = 8 * MIB + 1, 8 * MIB + 128 * KIB, 9 * MIB - 1, 12 * MIB + 17
BIG_LENGTHS = (BIG_1, BIG_EXACT, BIG_9, BIG_12)


def tiles(span, tile):
    return -(-span // tile)


def span_of(call):
    """the bytes the call scans: the document, or its range"""
    x = call.extra
    if "part" in x:
        return x["cut"] if x["part"] == 0 else call.doc.length - x["cut"]
    return call.doc.length


def kernel_of(call):
    """the kernel launch_fused picks for the call (use_fused / tokens_fused / launch_fused), None for the split pipeline, the kernel's own name for the two
    entry points that are no scan"""
    if call.op in OTHER_OPS:
        return {"validate_utf8_device": "k_validate_utf8", "string_parity_device": "k_string_parity"}[call.op]
    span = span_of(call)
    if not (call.pipeline == "fused" or (call.pipeline == "auto" and span <= AUTO_FUSED_BELOW)):
        return None
    small = span <= SMALL_BELOW
    if call.op in STAGE1_OPS:
        return "k_fused<0>" if small else "k_fused_pipelined<0>"
    if call.op in TOKEN_OPS:
        return "k_fused<0, tokens>" if small else "k_fused_pipelined<0, tokens>"
    assert call.op in MINIFY_OPS, call.op
    return "k_fused<1>" if small else "k_minify_onchip<8>"


def ntiles_of(call):
    """descriptors the call's kernel uses: its control words lie behind them.  0 for a call that takes no single-pass kernel"""
    k = kernel_of(call)
    if k not in SIX_KERNELS:
        return 0
    tile = TILE_ONCHIP if k == "k_minify_onchip<8>" else (TILE_PIPELINED if "pipelined" in k else TILE_SMALL)
    return tiles(span_of(call), tile)


# ---- sequences ------------------------------------------------------------------------------------------------------------------------------------
def _doc(length, k=0, kind=None):
    return Doc(kind or VALID[k % len(VALID)], length, 100 + k)


def _call(op, pipeline, doc, **extra):
    return Call(op, pipeline, doc, extra)


def _range_pair(op, pipeline, doc, cut):
    return [_call(op, pipeline, doc, part=0, cut=cut), _call(op, pipeline, doc, part=1, cut=cut)]


LADDER_A = 3
LADDER_STEPS = tuple(range(1, 19)) + (19, 40, 64)
_LADDER_OPS = ("stage1_device", "minify_device", "stage1_tokens_device")


def _ladder_length(t, k):
    """a length of t tiles of 16 KiB: one byte short of the border, on it, one byte behind the border in front"""
    return (t * TILE_SMALL - 1, t * TILE_SMALL, (t - 1) * TILE_SMALL + 1)[k % 3]


def overlap_ladder():
    """16 KiB-tile calls of A = 3 tiles and of A + k tiles in turn, for k = 1 .. 18 and 19, 40, 64, with stage 1, minify and the token variant interleaved:
    every one of the 18 control-word slots behind a short call's descriptors -- the second ticket counter, sixteen words out, among them -- has been a
    descriptor of the next call, and the long call's control words land on memory no short call ever touched."""
    seq = [_call("stage1_device", "fused", _doc(_ladder_length(LADDER_A, 0), 0))]
    for k in LADDER_STEPS:
        for j, op in enumerate(_LADDER_OPS):
            seq.append(_call(op, "fused", _doc(_ladder_length(LADDER_A + k, k), k)))
            seq.append(_call(_LADDER_OPS[(j + 1) % 3], "fused", _doc(_ladder_length(LADDER_A, k + j), k + j)))
    return seq


def kernel_round():
    """one context on the single-pass road: k_fused<0> -> k_minify_onchip<8> -> k_fused<0, tokens> -> k_fused_pipelined<0> -> k_fused<1> -> pipelined tokens
    -> k_fused<0>, a range pair and shard calls in between; ntiles goes 20, 193, [192, 73], 64, 65, 19, 17, 72, [64, 512], 130, 65, 18, 72, 2, 1"""
    big = _doc(BIG_12, 1)
    return [
        _call("stage1_device", "fused", _doc(19 * TILE_SMALL + 1, 0)),
        _call("minify_device", "fused", big),
        *_range_pair("stage1_range_device", "fused", big, 3 * MIB),       # [0, 3 MiB): 192 tiles of 16 KiB; [3 MiB, 12 MiB + 17): 73 of 128 KiB, begin > 0
        _call("stage1_tokens_device", "fused", _doc(64 * TILE_SMALL, 2)),
        _call("stage1_device", "fused", _doc(BIG_1, 3)),
        _call("stage1_shard_device", "fused", Doc("in_string_tail", 19 * TILE_SMALL - 1, 7), in_string=1),
        _call("minify_device", "fused", _doc(17 * TILE_SMALL - 1, 4)),
        _call("stage1_tokens_device", "fused", _doc(BIG_9, 5)),
        *_range_pair("minify_range_device", "fused", _doc(BIG_9, 5), 1 * MIB),  # 64 tiles, then 8 MiB - 1 behind begin = 1 MiB: 512 tiles of 16 KiB
        _call("minify_shard_device", "fused", _doc(BIG_EXACT, 6), in_string=0),
        _call("stage1_device", "fused", _doc(BIG_EXACT, 6)),              # 65 tiles of 128 KiB, the last one full
        _call("minify_shard_device", "fused", Doc("in_string_tail", 17 * TILE_SMALL + 1, 11), in_string=1),
        _call("stage1_shard_device", "fused", _doc(BIG_9, 5), in_string=0),
        _call("stage1_device", "fused", _doc(2 * TILE_SMALL, 8)),
        _call("string_parity_device", "fused", _doc(18 * TILE_SMALL + 1, 9)),
        _call("stage1_device", "fused", _doc(TILE_SMALL - 1, 10)),
    ]


def outcomes():
    """every way a call can end other than well -- an unclosed string, a control character inside a string, bad UTF-8, a list that does not fit -- each
    followed by a valid call with MORE tiles: a kernel that raises flags or stops emitting still counts itself out and cleans"""
    seq = []
    for k, (kind, t) in enumerate((("unclosed", 3), ("ctrl", 17), ("bad_utf8", 18))):
        bad = Doc(kind, _ladder_length(t, k), 200 + k)
        for j, op in enumerate(_LADDER_OPS):
            seq.append(_call(op, "fused", bad))
            seq.append(_call(_LADDER_OPS[(j + 1) % 3], "fused", _doc(_ladder_length(t + 1 + j, j), 20 + 3 * k + j)))
    seq += [_call("validate_utf8_device", "fused", Doc("bad_utf8", 18 * TILE_SMALL + 1, 203)), _call("stage1_device", "fused", _doc(19 * TILE_SMALL, 30))]
    dense = Doc("dense", 19 * TILE_SMALL - 1, 31)
    seq += [_call("stage1_device", "fused", dense, idx_words="n+2"), _call("stage1_tokens_device", "fused", dense, idx_words="n+2"),
            _call("minify_device", "fused", _doc(64 * TILE_SMALL + 1, 32))]
    # the same on the large-input kernels
    seq += [_call("stage1_device", "fused", Doc("dense", BIG_1, 33), idx_words="n+2"), _call("stage1_device", "fused", _doc(BIG_9, 34, "sparse")),
            _call("minify_device", "fused", Doc("unclosed", BIG_EXACT, 35)), _call("minify_device", "fused", _doc(BIG_9, 5)),
            _call("stage1_tokens_device", "fused", Doc("bad_utf8", BIG_1, 36)), _call("stage1_tokens_device", "fused", _doc(BIG_12, 1)),
            _call("stage1_device", "fused", Doc("ctrl", BIG_9, 37)), _call("stage1_device", "fused", _doc(BIG_12, 1))]
    return seq


ROADS_FIRST_CAPACITY = 1 * MIB


def roads():
    """fused -> split -> fused -> auto on one context made for 1 MiB documents; then its limit moves and a document arrives that makes
    ensure_scan_workspace re-allocate result, descriptors and control words (cleared once, by the host); then smaller documents again"""
    return [
        _call("stage1_device", "fused", _doc(3 * TILE_SMALL - 1, 40)),
        _call("minify_device", "split", _doc(19 * TILE_SMALL, 41)),
        _call("stage1_tokens_device", "fused", _doc(18 * TILE_SMALL, 42)),
        _call("stage1_device", "fused", _doc(BIG_1, 3), set_capacity=MAX_BYTES),   # 1 MiB of workspace -> 16 MiB
        _call("stage1_device", "auto", _doc(17 * TILE_SMALL + 1, 43)),              # AUTO: single pass up to 5 MiB
        _call("minify_device", "auto", _doc(BIG_EXACT, 6)),                         # ... the split pipeline beyond
        _call("stage1_tokens_device", "auto", _doc(BIG_9, 5)),
        _call("stage1_tokens_device", "auto", _doc(18 * TILE_SMALL - 1, 44)),
        _call("stage1_device", "split", _doc(BIG_12, 1)),
        _call("minify_device", "fused", _doc(2 * TILE_SMALL + 1, 45)),
        _call("minify_device", "fused", _doc(BIG_12, 1)),
        _call("validate_utf8_device", "auto", _doc(64 * TILE_SMALL - 1, 46)),
        _call("stage1_device", "auto", _doc(TILE_SMALL, 47)),
    ]


def parked_context():
    """the first ten calls of the ladder, for a context that was closed behind the kernel round and taken from the pool again"""
    return overlap_ladder()[:10]


def borders():
    """every length around a tile border -- T * 16 KiB - 1, T * 16 KiB, T * 16 KiB + 1 for T = 1, 2, 3, 17, 18, 19, 64 -- largest and smallest in turn, the
    three operations in turn: the last tile one byte long, full, or one byte short of full"""
    up = sorted(SMALL_LENGTHS)
    order = [n for pair in zip(reversed(up), up) for n in pair][: len(up)]
    return [_call(_LADDER_OPS[k % 3], "fused", _doc(n, 70 + k)) for k, n in enumerate(order)]


SEQUENCES = {"overlap_ladder": overlap_ladder, "kernel_round": kernel_round, "outcomes": outcomes, "roads": roads, "parked_context": parked_context,
             "borders": borders}

# test_back_to_back_without_a_host_round_trip: three stage-1 scans enqueued on one stream, nothing in between
BACK_TO_BACK = (
    (_doc(3 * TILE_SMALL - 1, 50), _doc(20 * TILE_SMALL + 1, 51), _doc(4 * TILE_SMALL, 52)),       # 3, 21 and 4 tiles of 16 KiB
    (_doc(3 * TILE_SMALL, 53), _doc(BIG_12, 1), _doc(18 * TILE_SMALL + 1, 54)),                    # 3 of 16 KiB, 97 of 128 KiB, 19 of 16 KiB
)
# test_host_entry_points_never_re_run: a length of every class, every broken kind, and what goes through the overlapped path in 9 MiB ranges
HOST_LENGTHS = (3 * TILE_SMALL - 1, 19 * TILE_SMALL + 1, 64 * TILE_SMALL, BIG_1, BIG_12)
HOST_DOCS = tuple(_doc(n, 60 + k) for k, n in enumerate(HOST_LENGTHS))
HOST_BROKEN = tuple(Doc(kind, 19 * TILE_SMALL + 1, 64) for kind in ("unclosed", "ctrl", "bad_utf8"))
HOST_OVERLAPPED = (Doc("sparse", BIG_12, 101), Doc("runs", BIG_12, 61), Doc("unclosed", BIG_EXACT, 35))
# test_a_traced_call_is_followed_by_a_right_one: the call in front, the traced one, the two behind it
TRACED = (Doc("dense", 3 * TILE_SMALL, 53), Doc("sparse", 18 * TILE_SMALL + 1, 54), Doc("runs", 64 * TILE_SMALL - 1, 55), Doc("dense", 19 * TILE_SMALL - 1, 31))


def all_calls():
    return [(name, i, c) for name, f in SEQUENCES.items() for i, c in enumerate(f())]


def all_documents():
    docs = {c.doc for _, _, c in all_calls()}
    docs.update(d for group in BACK_TO_BACK for d in group)
    docs.update(HOST_DOCS + HOST_BROKEN + HOST_OVERLAPPED + TRACED)
    return sorted(docs)
