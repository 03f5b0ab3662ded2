"""GPU tier (-m gpu): single-pass calls leave their workspace clean -- looked at on the device, behind every call.

A single-pass call is one dispatch: k_fused, k_fused_pipelined and k_minify_onchip clear nothing in front of themselves and trust that the kernel before
them left [tile descriptors][control words] all zero (sjgpu_fused.hip: leave_and_clean).  The control words lie behind THIS call's ntiles descriptors, so a
word left behind is another call's descriptor, later, for one order of call sizes; what it would cause -- a look-back that spins to its one-second
timeout, SJGPU_F_INTERNAL, and a host entry point that re-runs the call on the split pipeline and returns the right bytes -- no comparison of outputs sees.
The serial emulator checks the invariant (tests/host/test_kernels_emu.cpp: check_workspace_clean); which workgroup leaves last, whether another
workgroup's descriptor store can land behind the zeroing, minify's two ticket counters and kernels back to back on a stream exist on the hardware only.

Here: the call sequences of tests/workspace_cases.py (checked against the headers and the oracle on the CPU tier: tests/test_workspace_cases.py), and
behind EVERY call (1) its output against the oracle, (2) no SJGPU_F_INTERNAL and sjgpu_debug_gave_up_count still 0, (3) every word of the workspace
zero -- the whole allocation (sjgpu_debug_read_workspace), not only what this call used -- and the device's result equal to the one sjgpu_result gave,
(4) the allocation as large as the largest call so far needs.  Nothing here writes into the workspace, and no call can time out by design."""
import functools
import os

import numpy as np
import pytest

import checkers
import workspace_cases as W
from simdjson_amd import build, capi, corpus

pytestmark = pytest.mark.gpu

GUARD = 64          # elements of poison behind every exactly sized output
POISON8, POISON32 = 0x5A, 0x5A5A5A5A
SPLIT_KERNELS = {"stage1": "k_stage1_summarize+k_resolve_groups+k_resolve_segments+k_stage1_emit",
                 "tokens": "k_stage1_summarize<tokens>+k_resolve_groups+k_resolve_segments+k_stage1_emit<tokens>",
                 "minify": "k_minify_summarize+k_resolve_groups+k_resolve_segments+k_minify_emit"}


# ---- the oracle, once per document --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle():
    build.build_oracle()
    return checkers.Oracle()


@functools.lru_cache(maxsize=None)
def want_scan(doc):
    """(offsets, flags) of the raw scan of the document (an in_string_tail: of the tail, as the scan behind its 16-byte head gives them)"""
    idx, flags = _oracle().scan(W.oracle_input(doc))
    if doc.kind == "in_string_tail":
        idx = idx[idx >= len(W.HEAD)] - len(W.HEAD)
    idx = np.ascontiguousarray(idx, np.uint32)
    idx.setflags(write=False)
    return idx, flags


@functools.lru_cache(maxsize=None)
def want_minify(doc):
    err, out = _oracle().minify(W.oracle_input(doc))
    if doc.kind == "in_string_tail":
        assert bytes(out[: len(W.HEAD)]) == W.HEAD  # `[`, the quote and the string's first bytes: kept as they are
        out = out[len(W.HEAD):]
    return err, out


@functools.lru_cache(maxsize=None)
def want_utf8(doc):
    return _oracle().validate_utf8(W.make(doc))


_resident = {}


def resident(doc):
    """the document on the device (16-byte aligned: an allocation of its own), uploaded once"""
    import torch
    if doc not in _resident:
        _resident[doc] = torch.from_numpy(W.make(doc).copy()).cuda()
    return _resident[doc]


@pytest.fixture(scope="module", autouse=True)
def _release_documents():
    build.build_sjgpu()
    yield
    _resident.clear()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _parser(capacity=W.MAX_BYTES, pipeline="fused"):
    """a context whose small documents take the tile pipelines on the host-buffer road too (SJGPU_SMALL_DOCS=0: read when the context is made; the
    one-workgroup kernel for small documents keeps its descriptors in page-locked memory -- other state, not looked at here)"""
    old = os.environ.get("SJGPU_SMALL_DOCS")
    os.environ["SJGPU_SMALL_DOCS"] = "0"
    try:
        p = capi.DomParserImplementation(capacity)
    finally:
        if old is None:
            del os.environ["SJGPU_SMALL_DOCS"]
        else:
            os.environ["SJGPU_SMALL_DOCS"] = old
    p.set_pipeline(pipeline)
    return p


def poisoned(count, dtype):
    import torch
    return torch.full((int(count) + GUARD,), POISON32 if dtype == torch.int32 else POISON8, dtype=dtype, device="cuda")


def guard_intact(t, used):
    import torch
    return bool((t[int(used):] == (POISON32 if t.dtype == torch.int32 else POISON8)).all().item())


def first_diff(a, b):
    m = min(len(a), len(b))
    d = np.flatnonzero(np.asarray(a[:m]) != np.asarray(b[:m]))
    return (int(d[0]), int(a[d[0]]), int(b[d[0]])) if len(d) else ("len", len(a), len(b))


# ---- the look at the workspace ------------------------------------------------------------------------------------------------------------------------
def assert_workspace_clean(p, where, ntiles=None, prev_ntiles=None):
    """every word of the context's single-pass workspace is zero; -> (the device's result, words allocated)"""
    res, words = p.read_workspace()
    nz = np.flatnonzero(words)
    if len(nz):
        at = int(nz[0])
        what = ""
        if ntiles is not None and 0 <= at - ntiles < W.CTL_WORDS:
            what = f" = control word {at - ntiles} of this call"
        elif prev_ntiles is not None and 0 <= at - prev_ntiles < W.CTL_WORDS:
            what = f" = control word {at - prev_ntiles} of the call before"
        raise AssertionError(f"{where}: workspace word {at}{what} is {int(words[at]):#x} behind the kernel ({len(nz)} of {len(words)} words are not zero); "
                             f"this call's ntiles = {ntiles}, the previous call's = {prev_ntiles}; kernel: {p.profile_kernel()}")
    return res, len(words)


class State:
    """what a sequence carries from call to call"""

    def __init__(self, p, name):
        self.p, self.name = p, name
        self.checked = 0
        self.prev_ntiles = 0
        self.max_ntiles = 0
        self.gave_up_at_start = p.gave_up_count()
        self.ranges = {}     # (op, doc) -> what part 0 of a range pair hands to part 1
        self.kernels = {}    # kernel -> (smallest, largest ntiles)
        assert self.gave_up_at_start == 0, f"{name}: the context starts with {self.gave_up_at_start} calls that gave up"


def checked_call(p, entry, st):
    """Runs one entry of a sequence and checks it on the four points of the module's docstring."""
    import torch
    i, where = st.checked, f"{st.name}[{st.checked}] {entry.op} {entry.pipeline} {entry.doc}"
    doc, x = entry.doc, entry.extra
    a, buf, L, stream = W.make(doc), resident(doc), entry.doc.length, _stream()
    if "set_capacity" in x:
        assert p.set_capacity(x["set_capacity"]) == 0
    p.set_pipeline(entry.pipeline)
    kernel, ntiles = W.kernel_of(entry), W.ntiles_of(entry)
    whole, wflags = want_scan(doc)
    ctrl = bool(wflags & capi.F_UNESCAPED_CTRL)  # (the reference returns before anybody looks at the list: n and the offsets are not compared)

    # ---- the call, its result, (1) its output against the oracle ----
    if entry.op in ("stage1_device", "stage1_tokens_device", "stage1_shard_device"):
        tokens = entry.op == "stage1_tokens_device"
        n = len(whole)
        words = L + 3 if ctrl else {None: n + 3, "n+2": n + 2}[x.get("idx_words")]
        idx = poisoned(words, torch.int32)
        tok = poisoned(words, torch.uint8) if tokens else None
        if tokens:
            assert p.stage1_tokens_device(buf.data_ptr(), L, idx.data_ptr(), words, tok.data_ptr(), words, stream) == 0, where
        elif entry.op == "stage1_shard_device":
            p.stage1_shard_device(buf.data_ptr(), L, x["in_string"], idx.data_ptr(), words, stream)
        else:
            assert p.stage1_device(buf.data_ptr(), L, idx.data_ptr(), words, stream) == 0, where
        res = p.result(stream)
        assert guard_intact(idx, words) and (tok is None or guard_intact(tok, words)), f"{where}: a store behind idx_words = {words}"
        if words < n + 3:  # the list does not fit: the flag, the FULL count, nothing behind the capacity
            assert (res[0], res[1]) == (n, wflags | capi.F_IDX_OVERFLOW), (where, res, n, wflags)
        elif ctrl:
            assert res[1] == wflags, (where, res, wflags)
        else:
            assert (res[0], res[1]) == (n, wflags), (where, res, n, wflags)
            host = idx[: n + 3].cpu().numpy().view(np.uint32)
            assert np.array_equal(host[:n], whole), (where, first_diff(host[:n], whole))
            assert list(host[n:]) == [L, L, 0], (where, list(host[n:]))
            if tokens:
                got = tok[:n].cpu().numpy()
                assert np.array_equal(got, a[whole]), (where, first_diff(got, a[whole]))  # tok[i] == buf[idx[i]]
    elif entry.op in ("minify_device", "minify_shard_device"):
        oerr, oout = want_minify(doc)
        dst = poisoned(L, torch.uint8)
        if entry.op == "minify_shard_device":
            assert oerr == 0
            p.minify_shard_device(buf.data_ptr(), L, x["in_string"], dst.data_ptr(), stream)
        else:
            assert p.minify_device(buf.data_ptr(), L, dst.data_ptr(), stream) == 0, where
        res = p.result(stream)
        assert guard_intact(dst, L), f"{where}: a store behind dst + len"
        assert res[1] & (capi.F_IDX_OVERFLOW | capi.F_UNCLOSED_STRING) == (capi.F_UNCLOSED_STRING if oerr else 0), (where, res, oerr)
        if oerr:
            assert res[2] == 0, (where, res)  # sjgpu.h: out_len is 0 behind an unclosed string
        else:
            got = dst[: res[2]].cpu().numpy()
            assert res[2] == len(oout) and np.array_equal(got, oout), (where, res, len(oout), first_diff(got, oout))
    elif entry.op == "validate_utf8_device":
        assert p.validate_utf8_device(buf.data_ptr(), L, stream) == 0, where
        res = p.result(stream)
        assert bool(res[1] & capi.F_UTF8_ERROR) == (not want_utf8(doc)), (where, res)
    elif entry.op == "string_parity_device":
        parity = p.string_parity_device(buf.data_ptr(), L, stream)
        res = p.result(stream)
        assert parity == (wflags & 1) == (res[0] & 1), (where, parity, wflags, res)  # an odd number of unescaped quotes <=> the scan ends inside a string
    elif entry.op in ("stage1_range_device", "minify_range_device"):
        stage1 = entry.op == "stage1_range_device"
        key, cut = (entry.op, doc), x["cut"]
        oerr, oout = want_minify(doc)
        assert not ctrl and oerr == 0
        if x["part"] == 0:
            out = poisoned(len(whole) + 3, torch.int32) if stage1 else poisoned(L, torch.uint8)
            carry, before, begin, end = 0, 0, 0, cut
        else:
            out, carry, before = st.ranges.pop(key)
            begin, end = cut, L
        if stage1:
            p.stage1_range_device(buf.data_ptr(), begin, end, end < L, carry, before, out.data_ptr(), len(whole) + 3, stream)
        else:
            p.minify_range_device(buf.data_ptr(), begin, end, end < L, carry, before, out.data_ptr(), stream)
        res = p.result(stream)
        now = res[0] if stage1 else res[2]
        assert guard_intact(out, len(whole) + 3 if stage1 else L), f"{where}: a store behind the output"
        assert res[1] & ~(1 | capi.F_RANGE_CARRY) == 0 and before <= now <= (len(whole) if stage1 else len(oout)), (where, res)
        host = out[: now + (3 if stage1 and end == L else 0)].cpu().numpy()
        want = whole if stage1 else oout
        if stage1:
            host = host.view(np.uint32)
        # what the ranges so far have written is the whole scan's output up to there; behind the last range, all of it (and the sentinels)
        assert np.array_equal(host[:now], want[:now]), (where, first_diff(host[:now], want[:now]))
        if end == L:
            assert now == len(want) and res[1] & 1 == 0, (where, res, len(want))
            assert not stage1 or list(host[now:]) == [L, L, 0], (where, list(host[now:]))
        else:
            st.ranges[key] = (out, res[1] & (1 | capi.F_RANGE_CARRY), now)
    else:
        raise AssertionError(f"no such operation: {entry.op}")

    # ---- the road the plan says ----
    took = p.profile_kernel()
    if entry.op == "string_parity_device":
        pass  # (no scan: last_kernel stays what it was)
    elif kernel is None:
        assert p.last_pipeline() == "split" and took in SPLIT_KERNELS.values(), (where, took)
    else:
        assert took.split(" (")[0] == kernel, (where, took, kernel)
        if kernel in W.SIX_KERNELS:
            assert p.last_pipeline() == "fused", where
            lo, hi = st.kernels.get(kernel, (ntiles, ntiles))
            st.kernels[kernel] = (min(lo, ntiles), max(hi, ntiles))
    # ---- (2) nobody gave up ----
    assert res[1] & capi.F_INTERNAL == 0, f"{where}: SJGPU_F_INTERNAL ({took}, ntiles {ntiles}, the call before {st.prev_ntiles})"
    assert p.gave_up_count() == st.gave_up_at_start == 0, f"{where}: sjgpu_debug_gave_up_count = {p.gave_up_count()} ({took})"
    # ---- (3) the whole workspace is zero, and the accessor reads the live result ----
    dev_res, allocated = assert_workspace_clean(p, where, ntiles, st.prev_ntiles)
    assert dev_res == res, f"{where}: the device's result is {dev_res}, sjgpu_result gave {res}"
    # ---- (4) the allocation holds the largest call so far ----
    st.max_ntiles = max(st.max_ntiles, ntiles)
    assert allocated >= st.max_ntiles + W.CTL_WORDS, f"{where}: {allocated} words allocated, {st.max_ntiles} tiles + {W.CTL_WORDS} needed"
    st.prev_ntiles = ntiles if ntiles else st.prev_ntiles
    st.checked = i + 1
    return res


def run_sequence(p, name, seq):
    st = State(p, name)
    for entry in seq:
        checked_call(p, entry, st)
    assert st.checked == len(seq) and not st.ranges, (name, st.checked, len(seq))  # no entry skipped, no range pair left open
    assert p.gave_up_count() == 0
    print(f"{name}: {st.checked} calls checked; ntiles (smallest, largest) per kernel: {st.kernels}")
    return st


# ---- one test per sequence ----------------------------------------------------------------------------------------------------------------------------
def test_overlap_ladder():
    p = _parser()
    st = run_sequence(p, "overlap_ladder", W.overlap_ladder())
    assert set(st.kernels) == {"k_fused<0>", "k_fused<0, tokens>", "k_fused<1>"} and all(v == (3, 67) for v in st.kernels.values()), st.kernels
    p.close()


def test_kernel_round_and_a_parked_context():
    """sequence 2 (the six kernels in turn on one context), then sequence 5: the context is closed -- parked, with its workspace -- and the next parser
    takes it from the pool: same descriptors, same control words, and its give-up counter starts again at zero"""
    p = _parser()
    st = run_sequence(p, "kernel_round", W.kernel_round())
    assert set(st.kernels) == set(W.SIX_KERNELS), st.kernels
    words_before = len(p.read_workspace()[1])
    p.close()
    q = _parser()
    res, words = q.read_workspace()
    assert len(words) == words_before > W.CTL_WORDS and not words.any(), "the new parser did not get the parked context (or its workspace is not clean)"
    assert q.gave_up_count() == 0
    run_sequence(q, "parked_context", W.parked_context())
    q.close()


def test_outcomes():
    p = _parser()
    st = run_sequence(p, "outcomes", W.outcomes())
    assert set(st.kernels) == set(W.SIX_KERNELS), st.kernels
    p.close()


def test_roads():
    """fused -> split -> fused -> auto on a context of its own (the pool is emptied first: a parked context would bring its workspace), made for 1 MiB
    documents; the fourth call moves the limit and brings a document that makes ensure_scan_workspace re-allocate"""
    assert capi.load_library().sjgpu_pool_trim() >= 0
    p = _parser(capacity=W.ROADS_FIRST_CAPACITY)
    assert len(p.read_workspace()[1]) == 0  # no workspace yet
    seq, st, allocated = W.roads(), State(p, "roads"), []
    for entry in seq:
        checked_call(p, entry, st)
        allocated.append(len(p.read_workspace()[1]))
    assert st.checked == len(seq) and p.gave_up_count() == 0
    grow = next(i for i, c in enumerate(seq) if "set_capacity" in c.extra)
    assert len(set(allocated[:grow])) == 1 and len(set(allocated[grow:])) == 1 and allocated[grow] > allocated[0] >= 3 + W.CTL_WORDS, allocated
    print(f"roads: {st.checked} calls checked, {allocated[0]} -> {allocated[grow]} words; ntiles (smallest, largest) per kernel: {st.kernels}")
    p.close()


def test_borders():
    p = _parser()
    st = run_sequence(p, "borders", W.borders())
    assert set(st.kernels) == {"k_fused<0>", "k_fused<0, tokens>", "k_fused<1>"}, st.kernels
    p.close()


# ---- kernels back to back on one stream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", range(len(W.BACK_TO_BACK)))
def test_back_to_back_without_a_host_round_trip(group):
    """Three stage-1 scans of three documents enqueued on one stream into three exactly sized, poisoned lists -- no sjgpu_result, no wait, nothing of the
    host's between them (include/sjgpu.h: "Calls only enqueue; fetch the outcome with sjgpu_result()"; enqueue_stage1 reads no result): the second and the
    third kernel find what the kernel in front of them left, with no host round trip in which a late store could have settled.  One wait, then the three
    lists against the oracle and the look at the workspace.  (The largest of the three runs once in front, with its result fetched: the workspace is
    allocated for it, and no call of the three re-allocates under a kernel in flight.)"""
    import torch
    docs = W.BACK_TO_BACK[group]
    p, stream = _parser(), _stream()
    st = State(p, f"back_to_back[{group}]")
    checked_call(p, W.Call("stage1_device", "fused", max(docs, key=lambda d: d.length), {}), st)
    words_allocated = len(p.read_workspace()[1])
    lists = []
    for d in docs:
        n = len(want_scan(d)[0])
        lists.append(poisoned(n + 3, torch.int32))
        assert p.stage1_device(resident(d).data_ptr(), d.length, lists[-1].data_ptr(), n + 3, stream) == 0
    res = p.result(stream)  # the one wait: the third call's result
    for d, idx in zip(docs, lists):
        whole, wflags = want_scan(d)
        n = len(whole)
        assert wflags == 0 and guard_intact(idx, n + 3), d
        host = idx[: n + 3].cpu().numpy().view(np.uint32)
        assert np.array_equal(host[:n], whole) and list(host[n:]) == [d.length, d.length, 0], (d, first_diff(host[:n], whole), list(host[n:]))
    assert res == (len(want_scan(docs[-1])[0]), 0, 0) and p.gave_up_count() == 0, res
    nt = [W.ntiles_of(W.Call("stage1_device", "fused", d, {})) for d in docs]
    dev_res, allocated = assert_workspace_clean(p, f"back to back {nt}", nt[-1], nt[-2])
    assert dev_res == res and allocated == words_allocated
    p.close()


# ---- host buffers: the entry points that would re-run a call that gave up, without a word --------------------------------------------------------------
def _assert_same_host(p, orc, a, tag):
    err = p.stage1(a, capi.REGULAR)
    n = p.n_structural_indexes
    got = checkers.observable(a, 0, err, n, p.structural_indexes[: n + 3].copy())
    want = checkers.observable(a, 0, *orc.stage1(a, 0))
    assert got == want, f"stage1 mismatch {tag}: {got[:2]} {want[:2]}"
    assert p.gave_up_count() == 0, f"{tag}: sjgpu_stage1 re-ran its call ({p.profile_kernel()})"
    assert_workspace_clean(p, f"{tag}: sjgpu_stage1")
    gerr, gout = p.minify(a)
    oerr, oout = orc.minify(a)
    assert gerr == oerr and np.array_equal(gout, oout), f"minify mismatch {tag}: {gerr} {oerr} {first_diff(gout, oout) if gerr == oerr else ''}"
    assert p.gave_up_count() == 0, f"{tag}: sjgpu_minify re-ran its call ({p.profile_kernel()})"
    assert_workspace_clean(p, f"{tag}: sjgpu_minify")
    assert p.validate_utf8(a) == orc.validate_utf8(a), tag
    assert_workspace_clean(p, f"{tag}: sjgpu_validate_utf8")


def test_host_entry_points_never_re_run(monkeypatch):
    """sjgpu_stage1 / sjgpu_minify / sjgpu_parse re-run a single-pass call that raised SJGPU_F_INTERNAL on the split pipeline and return the right bytes
    (sjgpu_capi_host.hip, sjgpu_capi_stage2.hip, run_streamed in sjgpu_ctx.h): through them a call that took a second looks like any other.  The counter
    sees it.  Pipeline fused; a length of every class, valid and broken; then the overlapped path, in 9 MiB ranges (single-pass ranges with begin > 0,
    a result fetched behind each); then sjgpu_parse."""
    orc = _oracle()
    p = _parser()
    for doc in W.HOST_DOCS + W.HOST_BROKEN:
        _assert_same_host(p, orc, W.make(doc), f"host, {doc}")
    assert p.last_pipeline() == "fused"
    p.close()
    # a context with the defaults: documents between 64 KiB and 2 MiB have their offsets written straight into page-locked host memory (another retry site)
    p = capi.DomParserImplementation(W.MAX_BYTES)
    p.set_pipeline("fused")
    for doc in W.HOST_DOCS[1:3] + W.HOST_BROKEN:
        _assert_same_host(p, orc, W.make(doc), f"host, offsets written to host memory, {doc}")
    assert p.last_pipeline() == "fused"
    p.close()
    monkeypatch.setenv("SJGPU_STREAM_FROM_MB", "1")
    monkeypatch.setenv("SJGPU_STREAM_CHUNK_MB", "9")
    p = _parser()
    for doc in W.HOST_OVERLAPPED:  # ranges of 9 MiB and 3 MiB + 17 (128 KiB- and 16 KiB-tile kernels)
        _assert_same_host(p, orc, W.make(doc), f"overlapped host path, {doc}")
    assert p.last_pipeline() == "fused"
    p.close()
    monkeypatch.delenv("SJGPU_STREAM_FROM_MB")
    monkeypatch.delenv("SJGPU_STREAM_CHUNK_MB")
    p = _parser()
    a = corpus.twitter_like(9 << 20, 21)[0]
    e_want, t_want, s_want = orc.dom_parse(a)
    e_got, t_got, s_got = p.parse(a)
    assert e_got == e_want == 0 and np.array_equal(t_got, t_want) and bytes(s_got) == bytes(s_want)
    assert p.last_pipeline() == "fused" and p.gave_up_count() == 0
    assert_workspace_clean(p, "sjgpu_parse, 9 MiB")
    p.close()


def test_a_traced_call_is_followed_by_a_right_one():
    """sjgpu_debug_trace_stage1 runs the traced kernel (64 KiB tiles, the workspace cleared in front of it) and marks the workspace doubtful; the next call
    clears in front of its kernel instead of trusting.  What the traced kernel left is printed, not asserted -- ws_dirty exists so that nobody relies on
    it -- the call behind it, with more tiles, is right and leaves a clean workspace, and so does the one behind that, which trusts again."""
    import torch
    p = _parser()
    st = State(p, "traced")
    checked_call(p, W.Call("stage1_device", "fused", W.TRACED[0], {}), st)
    d = W.TRACED[1]
    idx = poisoned(d.length + 3, torch.int32)
    stamps = p.debug_trace_stage1(resident(d).data_ptr(), d.length, idx.data_ptr(), d.length + 3, 8)
    assert stamps.shape == (8, 8) and stamps[: W.tiles(d.length, 64 << 10), 1].all()  # every tile drew its ticket
    _, words = p.read_workspace()
    print(f"behind the traced call: {np.count_nonzero(words)} of {len(words)} workspace words are not zero")
    checked_call(p, W.Call("stage1_device", "fused", W.TRACED[2], {}), st)
    checked_call(p, W.Call("minify_device", "fused", W.TRACED[3], {}), st)
    assert st.checked == 3
    p.close()
