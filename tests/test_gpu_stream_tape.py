"""GPU tier (-m gpu): stage 2 of a document STREAM on the device -- sjgpu_stage2_many_device / sjgpu_parse_many (sjgpu_tape_many.hip) -- against the
reference's dom::parser::parse of every document's OWN bytes (the live libsjref.so where oracle/_ref/ travelled along, else the oracle, which is pinned
against it on the CPU tier): the code of the first broken document, the number of documents delivered, and for every document delivered its tape
slice word for word, its string records byte for byte and its table entry."""
import ctypes
import os

import numpy as np
import pytest

import checkers
import jsongen
import stream_cases
from simdjson_amd import _paths, build, capi

pytestmark = pytest.mark.gpu

CAP = 128 << 20
POISON = 0x5A
E_BADARG, E_OVERFLOW = -4, -5


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


@pytest.fixture(scope="module")
def orc():
    return checkers.Oracle()


@pytest.fixture(scope="module")
def ref():
    """the real reference where its library travelled along (and the host CPU can run an x86 kernel), else None"""
    if not checkers.have_reference_lib():
        return None
    r = checkers.Reference()
    return r if r.best_impl() else None


@pytest.fixture(scope="module")
def want_parse(orc, ref):
    if ref is not None:
        impl = ref.best_impl()
        return lambda d, md=1024: ref.dom_parse(impl, d, md)
    return lambda d, md=1024: orc.dom_parse(d, md)


class Resident:
    """a stream and its structural list in device memory, as sjgpu_stage1_device (mode None) or sjgpu_stage1_finish_device (a streaming mode) left them"""

    def __init__(self, p, data, mode=None):
        import torch
        self.torch = torch
        self.stream = torch.cuda.current_stream().cuda_stream
        a = checkers.as_u8(data)
        self.length = len(a)
        self.buf = torch.from_numpy(np.concatenate([a, np.zeros(16, np.uint8)])).cuda()  # (what lies behind the stream is not padding anybody relies on)
        self.idx = torch.zeros(len(a) + 16, dtype=torch.int32, device="cuda")
        assert p.stage1_device(self.buf.data_ptr(), len(a), self.idx.data_ptr(), len(a) + 3, self.stream) == 0
        self.n, flags, _ = p.result(self.stream)
        assert flags == 0, flags
        if mode is not None:
            err, self.n, _ = p.stage1_finish_device(self.buf.data_ptr(), len(a), mode, self.idx.data_ptr(), self.n, flags, self.stream)
            assert err == 0, err
            self.length = int(self.idx[self.n].item()) & 0xFFFFFFFF  # the list's sentinel: where the first token not kept stands


def many_device(p, res, max_depth=1024, tape_cap=None, str_cap=None, doc_cap=None, raw=False):
    """-> (code, documents, tape, string records, table[documents + 1]) -- outputs of exactly the capacities asked for (default: what always suffices)
    inside poisoned tensors whose poison must be intact around them and behind what the call reports"""
    torch = res.torch
    n = res.n
    tape_cap = 4 * n + 8 if tape_cap is None else tape_cap
    str_cap = 5 * (res.length // 3) + 256 if str_cap is None else str_cap
    doc_cap = n + 1 if doc_cap is None else doc_cap
    guard = 64
    tape = torch.full((tape_cap + 2 * guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    sbuf = torch.full((str_cap + 2 * guard,), POISON, dtype=torch.uint8, device="cuda")
    table = torch.full(((doc_cap + 2 * guard) * 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    docs, tw, sb = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = p.L.sjgpu_stage2_many_device(p.h, res.buf.data_ptr(), res.length, res.idx.data_ptr(), n, max_depth, tape.data_ptr() + 8 * guard, tape_cap,
                                      sbuf.data_ptr() + guard, str_cap, table.data_ptr() + 16 * guard, doc_cap, res.stream, ctypes.byref(docs), ctypes.byref(tw),
                                      ctypes.byref(sb))
    d, tw, sb = int(docs.value), int(tw.value), int(sb.value)
    th = tape.cpu().numpy().view(np.uint64)
    sh = sbuf.cpu().numpy()
    bh = table.cpu().numpy().view(np.uint32)
    written_docs = d + 1 if rc >= 0 and d else 0
    if rc < 0:
        tw = sb = 0
    # nothing in front of the arrays, nothing behind what was delivered (the string pass may have filled its buffer up to the capacity given when the
    # stream was broken or the call ended in an overflow: nothing beyond the capacity)
    assert (th[:guard] == 0x5A5A5A5A5A5A5A5A).all() and (th[guard + (tw if rc >= 0 else tape_cap):] == 0x5A5A5A5A5A5A5A5A).all(), "tape poison"
    if rc < 0:
        assert (th[guard: guard + tape_cap] == 0x5A5A5A5A5A5A5A5A).all(), "a call that failed wrote tape words"
    assert (sh[:guard] == POISON).all() and (sh[guard + str_cap:] == POISON).all(), "string buffer poison"
    if rc == 0:
        assert (sh[guard + sb: guard + str_cap] == POISON).all(), "string buffer poison behind the records delivered"
    assert (bh[: 4 * guard] == 0x5A5A5A5A).all() and (bh[4 * (guard + written_docs):] == 0x5A5A5A5A).all(), "table poison"
    if raw:
        return rc, d
    assert rc >= 0, (rc, p.last_error())
    return (rc, d, th[guard: guard + tw].copy(), sh[guard: guard + sb].copy(),
            bh[4 * guard: 4 * (guard + written_docs)].copy().view(capi.DOC_SPAN))


def check_delivered(got, stream, begins, want_parse, max_depth=1024, n=None, last_ends=None):
    """the documents delivered against the parse of each document's own bytes (the last one's end where the stream's: last_ends); -> (expected code,
    expected documents)"""
    code, d, tape, sbuf, table = got
    want_code, want_docs = 0, 0
    tapes, records = [], []
    ends = list(begins[1:]) + [len(stream) if last_ends is None else last_ends]
    for b, e in zip(begins, ends):
        ec, t, s = want_parse(stream[b:e], max_depth)
        if ec:
            want_code = ec
            break
        tapes.append(t)
        records.append(s)
        want_docs += 1
    assert (code, d) == (want_code, want_docs), (code, d, want_code, want_docs, bytes(stream[:200]))
    if d == 0:
        return want_code, want_docs
    assert len(table) == d + 1
    tb = np.concatenate([[0], np.cumsum([len(t) for t in tapes])]).astype(np.uint32)
    sb = np.concatenate([[0], np.cumsum([len(s) for s in records])]).astype(np.uint32)
    assert np.array_equal(table["tape_begin"], tb) and np.array_equal(table["string_begin"], sb), "table: tape / string offsets"
    assert np.array_equal(table["byte_begin"][:d], np.asarray(begins[:d], dtype=np.uint32)), "table: byte offsets"
    assert int(table["first_token"][0]) == 0 and (np.diff(table["first_token"].astype(np.int64)) > 0).all()
    if want_code == 0:
        assert int(table["byte_begin"][d]) == len(stream) and (n is None or int(table["first_token"][d]) == n)
    else:
        assert int(table["byte_begin"][d]) == begins[d]
    want_tape = np.concatenate(tapes)
    assert len(tape) == len(want_tape)
    if not np.array_equal(tape, want_tape):
        k = int(np.flatnonzero(tape != want_tape)[0])
        doc = int(np.searchsorted(tb, k, side="right")) - 1
        raise AssertionError(f"tape word {k} (document {doc}, word {k - int(tb[doc])}): {int(tape[k]):016x}, expected {int(want_tape[k]):016x}: {bytes(stream[begins[doc]:begins[doc] + 200])}")
    assert bytes(sbuf) == b"".join(bytes(s) for s in records), "string records"
    return want_code, want_docs


def run_stream(p, want_parse, docs, sep=b"\n", max_depth=1024):
    stream, begins = stream_cases.join(docs, sep)
    res = Resident(p, stream)
    return check_delivered(many_device(p, res, max_depth), stream, begins, want_parse, max_depth, res.n)


# ---- 1. valid streams ---------------------------------------------------------------------------------------------------------------------------
def test_two_thousand_random_documents(parser, want_parse):
    rng = np.random.default_rng(31)
    docs = stream_cases.valid_documents(rng, 2000)
    for sep in stream_cases.SEPARATORS:
        assert run_stream(parser, want_parse, docs, sep) == (0, 2000)


def test_the_reference_s_files_three_times_each(parser, want_parse):
    files = [open(os.path.join(_paths.REPO_ROOT, "tests", "golden", "jsonexamples", name), "rb").read() for name in ("twitter.json", "citm_catalog.json")]
    assert run_stream(parser, want_parse, [files[0]] * 3 + [files[1]] * 3) == (0, 6)
    assert run_stream(parser, want_parse, [files[0], files[1]] * 3, b"") == (0, 6)


def test_every_valid_number_as_a_root_scalar(parser, want_parse):
    texts = [t.encode() for t in jsongen.number_corner_cases()]
    valid = [t for t in texts if want_parse(t)[0] == 0]
    assert len(valid) > 400
    assert run_stream(parser, want_parse, valid) == (0, len(valid))


def test_two_hundred_thousand_small_records(parser, want_parse):
    """many token blocks of 4 096, sort tiles of 2 048 elements, string segments of 16 KiB, with documents that straddle each of those boundaries"""
    rng = np.random.default_rng(32)
    docs = stream_cases.small_records(rng, 200000)
    assert run_stream(parser, want_parse, docs) == (0, 200000)


def test_a_stream_of_one_document_is_the_single_document_s_tape(parser, want_parse):
    rng = np.random.default_rng(33)
    doc = b"[" + b",".join(stream_cases.valid_documents(rng, 300)) + b"]"
    res = Resident(parser, doc)
    code, d, tape, sbuf, table = many_device(parser, res)
    e1, t1, s1 = parser.parse(doc)
    assert (code, d, e1) == (0, 1, 0) and np.array_equal(tape, t1) and bytes(sbuf) == bytes(s1)
    check_delivered((code, d, tape, sbuf, table), doc, [0], want_parse)


def test_deep_documents_between_flat_ones(parser, want_parse):
    """both roads of the sort: documents nested 63, 64, 65 and 200 deep mixed with flat ones"""
    deep = [b"[" * d + b"1" + b"]" * d for d in (63, 64, 65, 200)]
    docs = [b'{"a":1}', deep[0], b"[1,2]", deep[1], b"3", deep[2], deep[3], b'"s"', b'{"a":[' * 100 + b"{}" + b"]}" * 100, b"[]"]
    for sep in stream_cases.SEPARATORS:
        assert run_stream(parser, want_parse, docs, sep) == (0, len(docs))


def test_streaming_final_with_a_last_document_cut_off(parser, want_parse):
    """finish() of streaming_final leaves the list of the COMPLETE documents with the buffer's length as its sentinel (json_structural_indexer.h:318-337):
    the tokens of a last document that is cut off are not in it, and every document in front of it comes back"""
    rng = np.random.default_rng(34)
    docs = stream_cases.small_records(rng, 3000)
    stream, begins = stream_cases.join(docs, b"\n")
    cut = stream + b'\n{"id":1,"tags":["a",'
    res = Resident(parser, cut, mode=checkers.MODES["streaming_final"])
    assert res.length == len(cut)
    got = many_device(parser, res)
    assert check_delivered(got, cut, begins, want_parse, n=res.n, last_ends=len(stream)) == (0, 3000)


# ---- 2. one broken document ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 500])
def test_one_broken_document(parser, want_parse, count):
    rng = np.random.default_rng(35 + count)
    valid = stream_cases.valid_documents(rng, count)
    seen = set()
    for where in sorted({0, count // 2, count - 1}):
        for k, (_, bad) in enumerate(stream_cases.broken_documents()):
            docs = list(valid)
            docs[where] = bad
            code, d = run_stream(parser, want_parse, docs, stream_cases.SEPARATORS[k % 3])
            assert d == where and code != 0, (bad, code, d)
            seen.add(code)
    assert seen == {3, 5, 6, 7, 8, 9, 10}, seen


@pytest.mark.parametrize("max_depth", [1, 2, 3, 16])
def test_nesting_beyond_max_depth(parser, want_parse, max_depth):
    flat = [b"1", b"[]", b"{}", b'"s"', b"true"] + ([b"[1]", b'{"a":2}'] if max_depth > 1 else [])
    for count in (1, 2, 500):
        for where in sorted({0, count // 2, count - 1}):
            docs = [flat[k % len(flat)] for k in range(count)]
            docs[where] = stream_cases.too_deep(max_depth)
            assert run_stream(parser, want_parse, docs, b"\n", max_depth) == (4, where)


# ---- 3. hand-written lists ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", stream_cases.HAND_WRITTEN, ids=[r[0].decode() or "empty" for r in stream_cases.HAND_WRITTEN])
def test_hand_written_table(parser, want_parse, row):
    stream, max_depth, want_docs, want_code = row
    if not stream:
        import torch
        buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
        docs = ctypes.c_uint32(7)
        rc = parser.L.sjgpu_stage2_many_device(parser.h, buf.data_ptr(), 0, buf.data_ptr(), 0, max_depth, buf.data_ptr(), 4, buf.data_ptr(), 4, buf.data_ptr(), 1, None,
                                               ctypes.byref(docs), None, None)
        assert (rc, docs.value) == (want_code, want_docs)
        return
    res = Resident(parser, stream)
    code, d, tape, sbuf, table = many_device(parser, res, max_depth)
    assert (d, code) == (want_docs, want_code)
    for k in range(d):  # the documents delivered: the parse of the bytes the table delimits
        b, e = int(table["byte_begin"][k]), int(table["byte_begin"][k + 1])
        ec, t, s = want_parse(stream[b:e], max_depth)
        assert ec == 0 and np.array_equal(tape[int(table["tape_begin"][k]): int(table["tape_begin"][k + 1])], t)
        assert bytes(sbuf[int(table["string_begin"][k]): int(table["string_begin"][k + 1])]) == bytes(s)


def test_stray_close_leaves_the_first_document_intact(parser, want_parse):
    """`{"a":1}} {"b":2}` with a first document of several thousand tokens and several levels: sorted by level, the stray bracket finds an opening
    bracket of the FIRST document -- which is why a broken stream is run again up to the broken document"""
    rng = np.random.default_rng(36)
    stream = stream_cases.stray_close_behind_a_large_document(rng, 2000)
    first = stream[: stream.index(b"} {")]
    res = Resident(parser, stream)
    code, d, tape, sbuf, table = many_device(parser, res)
    assert (d, code) == (1, 3) and int(table["byte_begin"][1]) == len(first)
    ec, t, s = want_parse(first)
    assert ec == 0 and np.array_equal(tape, t) and bytes(sbuf) == bytes(s)


# ---- 4. contract ------------------------------------------------------------------------------------------------------------------------------------
def test_exact_capacities_and_one_short(parser, want_parse):
    rng = np.random.default_rng(37)
    docs = stream_cases.small_records(rng, 700)
    stream, begins = stream_cases.join(docs, b"\n")
    res = Resident(parser, stream)
    code, d, tape, sbuf, table = many_device(parser, res)
    assert (code, d) == (0, 700)
    tw, sb = len(tape), len(sbuf)
    exact = many_device(parser, res, tape_cap=tw, str_cap=sb, doc_cap=d + 1)
    check_delivered(exact, stream, begins, want_parse, n=res.n)
    assert many_device(parser, res, tape_cap=tw - 1, str_cap=sb, doc_cap=d + 1, raw=True)[0] == E_OVERFLOW
    assert many_device(parser, res, tape_cap=tw, str_cap=sb - 1, doc_cap=d + 1, raw=True)[0] == E_OVERFLOW
    assert many_device(parser, res, tape_cap=tw, str_cap=sb, doc_cap=d, raw=True) == (E_OVERFLOW, d + 1)  # ... and says how many entries it needs


def test_misaligned_pointers(parser):
    import torch
    res = Resident(parser, b'{"a":1} {"b":2}')
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    base = out.data_ptr()
    docs = ctypes.c_uint32(0)

    def call(buf=res.buf.data_ptr(), idx=res.idx.data_ptr(), tape=base, table=base + 2048):
        return parser.L.sjgpu_stage2_many_device(parser.h, buf, res.length, idx, res.n, 1024, tape, 64, base + 1024, 512, table, 8, res.stream, ctypes.byref(docs), None, None)
    assert call() == 0 and docs.value == 2
    assert call(buf=res.buf.data_ptr() + 8) == E_BADARG
    assert call(idx=res.idx.data_ptr() + 2) == E_BADARG
    assert call(tape=base + 4) == E_BADARG
    assert call(table=base + 2048 + 8) == E_BADARG


# ---- 5. the host entry point and the Python views ---------------------------------------------------------------------------------------------------
def test_parse_many_equals_the_device_entry_point(parser, want_parse):
    rng = np.random.default_rng(38)
    for docs in (stream_cases.valid_documents(rng, 300), stream_cases.valid_documents(rng, 40) + [b'{"a":tru}'] + stream_cases.valid_documents(rng, 5)):
        stream, begins = stream_cases.join(docs, b"\n")
        code, d, tape, sbuf, table = many_device(parser, Resident(parser, stream))
        rc, d2, views, (tape2, sbuf2, table2) = parser.parse_many(stream)
        assert (rc, d2) == (code, d) and np.array_equal(tape2, tape) and np.array_equal(sbuf2, sbuf) and np.array_equal(table2, table)
        assert len(views) == d
        for k, (t, s) in enumerate(views):
            assert np.array_equal(t, tape[int(table["tape_begin"][k]): int(table["tape_begin"][k + 1])])
            assert np.array_equal(s, sbuf[int(table["string_begin"][k]): int(table["string_begin"][k + 1])])
            ec, tw, sw = want_parse(stream[begins[k]: begins[k + 1] if k + 1 < len(begins) else len(stream)])
            assert ec == 0 and np.array_equal(t, tw) and bytes(s) == bytes(sw)
    assert parser.parse_many(b"")[:2] == (13, 0)
