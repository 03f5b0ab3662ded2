"""CPU tier: what tests/workspace_cases.py -- the plan of tests/test_gpu_workspace.py -- claims about itself.  Every document is of the kind it says
(the oracle decides, here and only here); the tile sizes, the small-input limit, AUTO's limit and the number of control words the plan works with are the
ones in sjgpu_internal.h / sjgpu_ctx.h, read out of the headers; the overlap ladder really puts every control-word slot of a short call under a
descriptor of the next call; every length lies on the side of the small-input limit it is meant for; and the calls reach the six single-pass kernels,
each of them, and nothing else that is single-pass."""
import collections
import os
import re

import numpy as np
import pytest

import checkers
import workspace_cases as W
from simdjson_amd import _paths

CSRC = os.path.join(_paths.PKG_DIR, "csrc")


def _constants(header, names):
    """the `constexpr <type> NAME = <expression>;` lines of a header, evaluated in their order (the expressions are products, shifts and earlier names)"""
    text = open(os.path.join(CSRC, header)).read()
    env = {}
    for m in re.finditer(r"constexpr\s+(?:uint32_t|uint64_t|size_t|u32|u64)\s+(\w+)\s*=\s*([^;]+);", text):
        expr = re.sub(r"\b(?:uint64_t|uint32_t|size_t)\(([^()]*)\)", r"(\1)", m.group(2))
        try:
            env[m.group(1)] = int(eval(expr, {"__builtins__": {}}, dict(env)))  # noqa: S307 -- the project's own header
        except Exception:  # noqa: BLE001 -- an expression of other things (sizeof, ~): not one of ours
            continue
    assert all(n in env for n in names), [n for n in names if n not in env]
    return env


@pytest.fixture(scope="module")
def hdr():
    h = _constants("sjgpu_internal.h", ("CHUNK_BYTES", "FUSED_WAVE_CHUNKS", "ONCHIP_WAVE_CHUNKS", "FUSED_TILE_BYTES", "ONCHIP_TILE_BYTES", "FUSED_SMALL_BELOW",
                                        "FUSED_WORKSPACE_EXTRA_WORDS", "RANGE_ALIGN"))
    h.update({k: v for k, v in _constants("sjgpu_ctx.h", ("AUTO_FUSED_BELOW", "AUTO_FUSED_FROM", "AUTO_FUSED_FROM_MINIFY")).items() if k.startswith("AUTO_")})
    # the three tile sizes: k_fused one chunk per wave, four waves; the large-input kernels EIGHT waves per workgroup by default (launch_fused: pipe_waves,
    # minify_waves) -- twice the four-wave tiles the header names
    h["small"] = h["FUSED_TILE_BYTES"] // h["FUSED_WAVE_CHUNKS"]
    h["pipelined"] = 8 * h["FUSED_WAVE_CHUNKS"] * h["CHUNK_BYTES"]
    h["onchip"] = 8 * h["ONCHIP_WAVE_CHUNKS"] * h["CHUNK_BYTES"]
    return h


def test_the_plan_s_constants_are_the_headers(hdr):
    assert (W.TILE_SMALL, W.TILE_PIPELINED, W.TILE_ONCHIP) == (hdr["small"], hdr["pipelined"], hdr["onchip"]) == (16 << 10, 128 << 10, 64 << 10)
    assert hdr["pipelined"] == 2 * hdr["FUSED_TILE_BYTES"] and hdr["onchip"] == 2 * hdr["ONCHIP_TILE_BYTES"]
    assert W.SMALL_BELOW == hdr["FUSED_SMALL_BELOW"] and W.AUTO_FUSED_BELOW == hdr["AUTO_FUSED_BELOW"] and W.CTL_WORDS == hdr["FUSED_WORKSPACE_EXTRA_WORDS"]
    # AUTO comes back to the single-pass kernels far beyond anything here: above 5 MiB every AUTO call of the plan is a split call, as kernel_of says
    assert min(hdr["AUTO_FUSED_FROM"], hdr["AUTO_FUSED_FROM_MINIFY"]) > W.MAX_BYTES
    # draw_ticket: the odd workgroups' counter lies 32 u32 words behind the first one -- u64 word 16 of the 18
    fused = open(os.path.join(CSRC, "sjgpu_fused.hip")).read()
    assert "atomicAdd(ticket + 32u * odd, 1u)" in fused and W.SECOND_TICKET_WORD == 32 * 4 // 8 < W.CTL_WORDS


def test_every_document_is_of_its_kind():
    orc = checkers.Oracle()
    docs = W.all_documents()
    assert {d.kind for d in docs} == set(W.KINDS)
    for d in docs:
        a = W.make(d)
        assert len(a) == d.length <= W.MAX_BYTES and a.dtype == np.uint8, d
        x = W.oracle_input(d)
        _, flags = orc.scan(x)
        err = orc.stage1(x, 0)[0]
        assert (flags, err) == W.KINDS[d.kind], (d, flags, err)
        assert orc.validate_utf8(x) == (d.kind != "bad_utf8"), d
        assert (orc.minify(x)[0] != 0) == (d.kind == "unclosed"), d
        if d.kind == "in_string_tail":  # the head ends inside a string: the tail alone is another text
            assert len(x) == d.length + 16 and orc.scan(W.HEAD)[1] == W.F_UNCLOSED_STRING


def test_the_runs_cross_every_border():
    """the `runs` kind: 200 backslashes, 100 on either side of every 16 KiB border (so of every 64 KiB and 128 KiB border too) -- the 64 bytes in front of a
    tile do not settle its escape state"""
    for d in (d for d in W.all_documents() if d.kind == "runs"):
        a = W.make(d)
        borders = list(range(W.TILE_SMALL, d.length - 512, W.TILE_SMALL))
        assert borders or d.length <= W.TILE_SMALL + 512, d
        for b in borders:
            assert (a[b - 100: b + 100] == ord("\\")).all() and a[b - 101] != ord("\\") and a[b + 100] == ord('"'), (d, b)


def test_lengths_by_tile_count(hdr):
    lengths = {c.doc.length for _, _, c in W.all_calls()} | {d.length for g in W.BACK_TO_BACK for d in g} | set(W.HOST_LENGTHS)
    small = sorted(n for n in lengths if n <= 8 << 20)
    big = sorted(n for n in lengths if n > 8 << 20)
    # every length above 8 MiB is above the small-input limit, every other one is not; nothing beyond 13 MiB
    assert all(n > hdr["FUSED_SMALL_BELOW"] for n in big) and all(n <= hdr["FUSED_SMALL_BELOW"] for n in small) and max(big) <= 13 << 20
    assert set(big) == {(8 << 20) + 1, (8 << 20) + (128 << 10), (9 << 20) - 1, (12 << 20) + 17} == set(W.BIG_LENGTHS)
    # around every border of T = 1, 2, 3, 17, 18, 19, 64 tiles of 16 KiB: one byte short, the border, one byte behind -- T, T and T + 1 tiles
    for t in (1, 2, 3, 17, 18, 19, 64):
        for d, want in ((-1, t), (0, t), (1, t + 1)):
            n = t * hdr["small"] + d
            assert n in lengths and W.tiles(n, hdr["small"]) == want, (t, d)
    assert set(W.SMALL_LENGTHS) <= lengths
    # 12 MiB + 17: an odd tile count for either large tile size, 9 MiB - 1 an even one; with minify's two ticket streams both parities matter
    assert [W.tiles(W.BIG_12, hdr[k]) % 2 for k in ("pipelined", "onchip")] == [1, 1] and [W.tiles(W.BIG_9, hdr[k]) % 2 for k in ("pipelined", "onchip")] == [0, 0]
    assert W.tiles(W.BIG_EXACT, hdr["pipelined"]) * hdr["pipelined"] == W.BIG_EXACT  # the last tile full
    # ranges begin at a multiple of the range alignment, and the second range begins behind 0
    cuts = [c.extra["cut"] for _, _, c in W.all_calls() if "part" in c.extra]
    assert cuts and all(cut > 0 and cut % hdr["RANGE_ALIGN"] == 0 for cut in cuts)


def _ntiles(call, hdr):
    """ntiles_of, recomputed from the call's span with the header's tile sizes"""
    k = W.kernel_of(call)
    if k not in W.SIX_KERNELS:
        return 0
    return W.tiles(W.span_of(call), hdr["onchip"] if k == "k_minify_onchip<8>" else (hdr["pipelined"] if "pipelined" in k else hdr["small"]))


def test_the_ladder_covers_every_control_word(hdr):
    seq = W.overlap_ladder()
    assert all(c.pipeline == "fused" and c.doc.length <= hdr["FUSED_SMALL_BELOW"] for c in seq)
    nt = [_ntiles(c, hdr) for c in seq]
    assert nt == [W.ntiles_of(c) for c in seq]
    A = W.LADDER_A
    assert A == 3 and nt[0] == A
    # (A, A + k) and (A + k, A) for every k: the short call's control words desc[A .. A + 17] are descriptors of the long call as soon as k >= their
    # offset + 1, so k = 1 .. 18 puts them under descriptors one more at a time, the second ticket counter (offset 16) from k = 17 on
    up = {b - a for a, b in zip(nt, nt[1:]) if a == A}
    down = {a - b for a, b in zip(nt, nt[1:]) if b == A}
    assert set(range(1, 19)) | {19, 40, 64} == up == down
    assert W.SECOND_TICKET_WORD + 1 in up and hdr["FUSED_WORKSPACE_EXTRA_WORDS"] in up
    # each pair with each of the three operations on either side
    ops = {(a.op, b.op) for a, b in zip(seq, seq[1:])}
    assert {x for x, _ in ops} == {y for _, y in ops} == {"stage1_device", "minify_device", "stage1_tokens_device"}
    for k in W.LADDER_STEPS:
        longs = {c.op for c, n in zip(seq, nt) if n == A + k}
        assert longs == {"stage1_device", "minify_device", "stage1_tokens_device"}, k
    assert W.parked_context() == seq[:10] and len({W.ntiles_of(c) for c in W.parked_context()}) >= 3


def test_every_outcome_is_followed_by_a_valid_call_with_more_tiles():
    seq = W.outcomes()
    odd = [i for i, c in enumerate(seq) if c.doc.kind not in W.VALID or "idx_words" in c.extra]
    assert {seq[i].doc.kind for i in odd} == {"unclosed", "ctrl", "bad_utf8", "dense"} and any("idx_words" in seq[i].extra for i in odd)
    for i in odd:
        j = next(j for j in range(i + 1, len(seq)) if seq[j].doc.kind in W.VALID and "idx_words" not in seq[j].extra)
        assert j <= i + 2 and W.ntiles_of(seq[j]) > W.ntiles_of(seq[i]), (i, seq[i], seq[j])
    # on the small-input kernels and on the large-input ones
    assert {W.kernel_of(seq[i]) for i in odd} >= {"k_fused<0>", "k_fused<0, tokens>", "k_fused<1>", "k_fused_pipelined<0>", "k_fused_pipelined<0, tokens>",
                                                  "k_minify_onchip<8>"}


def test_no_entry_is_unreachable(hdr):
    """each (op, pipeline, span) mapped to the kernel launch_fused / use_fused pick for it: the single-pass kernels reached are exactly the six"""
    reached = collections.Counter()
    for name, i, c in W.all_calls():
        assert c.op in W.STAGE1_OPS + W.TOKEN_OPS + W.MINIFY_OPS + W.OTHER_OPS and c.pipeline in ("fused", "split", "auto"), (name, i)
        assert set(c.extra) <= {"idx_words", "in_string", "part", "cut", "set_capacity"}, (name, i)
        k = W.kernel_of(c)
        # use_fused / tokens_fused (sjgpu_ctx.h), launch_fused (sjgpu_fused.hip), with the header's numbers
        span = W.span_of(c)
        if c.op not in W.OTHER_OPS:
            fused = c.pipeline == "fused" or (c.pipeline == "auto" and span <= hdr["AUTO_FUSED_BELOW"])
            assert (k is not None) == fused, (name, i)
            if fused:
                assert ("pipelined" in k or "onchip" in k) == (span > hdr["FUSED_SMALL_BELOW"]), (name, i, k)
                assert ("tokens" in k) == (c.op in W.TOKEN_OPS) and (k in ("k_fused<1>", "k_minify_onchip<8>")) == (c.op in W.MINIFY_OPS), (name, i, k)
        reached[k] += 1
        assert W.ntiles_of(c) == _ntiles(c, hdr), (name, i)
    assert {k for k in reached if k is not None and k.startswith(("k_fused", "k_minify"))} == set(W.SIX_KERNELS) and len(W.SIX_KERNELS) == 6
    assert reached[None] >= 4 and reached["k_validate_utf8"] >= 2 and reached["k_string_parity"] >= 1  # the split pipeline and the two other kernels between them
    # the kernel round: the seven kernels in the order the issue names, on one context, its pipeline fused throughout
    seq = W.kernel_round()
    assert all(c.pipeline == "fused" for c in seq)
    order = [W.kernel_of(c) for c in seq]
    want = ["k_fused<0>", "k_minify_onchip<8>", "k_fused<0, tokens>", "k_fused_pipelined<0>", "k_fused<1>", "k_fused_pipelined<0, tokens>", "k_fused<0>"]
    it = iter(order)
    assert all(k in it for k in want), order  # a subsequence
    ups = [b > a for a, b in zip([W.ntiles_of(c) for c in seq], [W.ntiles_of(c) for c in seq][1:])]
    assert ups.count(True) >= 4 and ups.count(False) >= 4
    # every sequence holds what the issue asks for
    ops = {c.op for _, _, c in W.all_calls()}
    assert ops == set(W.STAGE1_OPS + W.TOKEN_OPS + W.MINIFY_OPS + W.OTHER_OPS)
    for op in ("stage1_shard_device", "minify_shard_device"):  # shards that begin outside a string and inside one
        assert {c.extra["in_string"] for _, _, c in W.all_calls() if c.op == op} == {0, 1}, op
    assert all((c.doc.kind == "in_string_tail") == (c.extra.get("in_string") == 1) for _, _, c in W.all_calls())
    assert [c.pipeline for c in W.roads()][:5] == ["fused", "split", "fused", "fused", "auto"] and {c.pipeline for c in W.roads()} == {"fused", "split", "auto"}
    grow = next(c for c in W.roads() if "set_capacity" in c.extra)
    assert W.roads()[0].doc.length <= W.ROADS_FIRST_CAPACITY < grow.doc.length <= grow.extra["set_capacity"]


def test_the_summary_s_table():
    """largest and smallest ntiles per kernel over the whole plan (the figures the pull request's summary quotes)"""
    seen = {}
    for _, _, c in W.all_calls():
        k = W.kernel_of(c)
        if k in W.SIX_KERNELS:
            lo, hi = seen.get(k, (1 << 30, 0))
            seen[k] = (min(lo, W.ntiles_of(c)), max(hi, W.ntiles_of(c)))
    print(seen)
    assert seen == {"k_fused<0>": (1, 192), "k_fused<0, tokens>": (2, 67), "k_fused<1>": (1, 512), "k_fused_pipelined<0>": (65, 97),
                    "k_fused_pipelined<0, tokens>": (65, 97), "k_minify_onchip<8>": (130, 193)}
