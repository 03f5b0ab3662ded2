"""GPU tier (-m gpu): every device-resident entry point on a CALLER'S stream, its inputs complete late, its outputs consumed without a host wait.

include/sjgpu.h promises that each of these calls takes the caller's hipStream_t and that its work is ordered with whatever else the caller enqueued there.
Every other GPU module hands over torch's current stream with no stream context active -- the legacy NULL stream -- with inputs long complete and outputs
read after a wait.  Here tests/stream_order.py's late_call() makes each call on a side stream (non-blocking: it does not synchronise with the NULL stream)
whose inputs still hold decoys when the call is made, while the NULL stream is busy for twice as long; see that module for what the probe can see.

Expected values never come from the library on another stream: the oracle (or the live reference where its library travelled along) gives the structural
lists, flags, minified bytes, verdicts, depths, string buffers, tapes and document tables; the Python models (pointer, path, rows, lists, fields, cast) run over
those tapes give the columns.

TABLE has one entry per method of capi.DomParserImplementation that takes a `stream`; tests/test_stream_order_cases.py (CPU tier) fails when a method is in
neither TABLE nor EXEMPT."""
import functools
import json
import time

import numpy as np
import pytest

import cast_model
import checkers
import fields_model
import path_cases
import pointer_model
import stream_cases
import stream_order as so
import test_gpu_casts
import test_gpu_fields
import test_gpu_lists
import test_gpu_paths
import test_gpu_query
import test_gpu_rows
from simdjson_amd import build, capi, corpus
from test_casts_emu import cycled, random_cells

pytestmark = pytest.mark.gpu

CAP = 16 << 20
SEED = 7
RANGE = 1 << 20
HEAD = b'["' + b"x" * 14  # sixteen bytes that open a string: in front of a shard that begins inside one, for the oracle
KEY_NAMES = [b"id", b"text", b"user", b"name", b"indices", b"not_there"]
POINTERS = [b"", b"/0", b"/5", b"/7", b"/9", b"/0/x"]  # over the amazon records: the record, a string, the rating (a double), the reviews (an integer), misses
PATHS = [b"$[*]", b"$[5]", b"$.x[*]"]
USERS, HASHTAGS = b"$.statuses[*].user", b"$.statuses[*].user.entities.hashtags"

EXEMPT = {
    "Comm.gather_indices": "needs RCCL and one process per rank: tests/gpu_comm_worker.py runs it on a stream of its own",
    "result": "no work of its own: every stage-1, minify, validate_utf8, parity, shard and range case fetches its outcome with result(stream)",
}


@functools.lru_cache(maxsize=None)
def documents():
    """every document the table's inputs are made of (seeded) -> {name: uint8 array}"""
    return {"twitter_like": corpus.twitter_like(2 << 20, SEED)[0], "amazon_ndjson": corpus.amazon_ndjson(1 << 20, SEED)[0],
            "amazon_ndjson_2": corpus.amazon_ndjson(512 << 10, SEED + 1)[0], "large_random": corpus.large_random(1 << 20, SEED)[0]}


def line_begins(stream):
    """where the documents of an NDJSON stream begin (every line is a document, the last one ends with a newline)"""
    ends = np.flatnonzero(np.asarray(stream) == 0x0A)
    assert int(ends[-1]) == len(stream) - 1
    return [0] + [int(e) + 1 for e in ends[:-1]]


def stream_tapes(parse, stream, idx):
    """the tapes, string records and document table sjgpu_stage2_many_device must deliver: the parse of every document's own bytes, side by side"""
    begins = line_begins(stream)
    tapes, records = [], []
    for b, e in zip(begins, begins[1:] + [len(stream)]):
        ec, t, s = parse(stream[b:e])
        assert ec == 0
        tapes.append(t)
        records.append(s)
    table = np.zeros(len(begins) + 1, capi.DOC_SPAN)
    table["byte_begin"] = begins + [len(stream)]
    table["first_token"] = np.searchsorted(idx, table["byte_begin"])
    table["tape_begin"] = np.concatenate([[0], np.cumsum([len(t) for t in tapes])])
    table["string_begin"] = np.concatenate([[0], np.cumsum([len(s) for s in records])])
    return np.concatenate(tapes), np.concatenate(records), table


# ---- the world: documents, what the checkers say about them, and the inputs in device memory ---------------------------------------------------------
class LateTapes:
    """tapes, string records and table as late inputs: the real document's (with their host copies, T, for the models) over the decoy document's"""

    def __init__(self, real, decoy):
        self.T = test_gpu_query.Tapes(*real)
        self.tape, self.sbuf, self.table = so.Late(real[0], decoy[0]), so.Late(real[1], decoy[1], pad=16), so.Late(real[2], decoy[2])
        self.inputs = [self.tape, self.sbuf, self.table]
        assert not np.array_equal(real[0], decoy[0]), "the decoy's tape is the real one"

    def args(self):
        return self.tape.ptr, len(self.T.tape), self.sbuf.ptr, len(self.T.sbuf), self.table.ptr, self.T.docs


class Doc:
    """one document, its decoy, the oracle's structural list of both (the same), and buffer + list as late inputs"""

    def __init__(self, orc, data, decoy=None):
        self.a = np.ascontiguousarray(data, np.uint8)
        self.decoy = so.decoy_document(self.a) if decoy is None else decoy
        self.L = len(self.a)
        self.idx, self.flags = orc.scan(self.a)
        didx, dflags = orc.scan(self.decoy)
        assert self.flags == dflags == 0 and np.array_equal(self.idx, didx), "a decoy keeps the structural list"
        self.n = len(self.idx)
        self.list = np.concatenate([self.idx, np.array([self.L, self.L, 0], np.uint32)]).astype(np.uint32)
        self.buf = so.Late(self.a, self.decoy, pad=64)
        self.idx_in = so.Late(self.list)


class World:
    def __init__(self, orc, parse):
        import torch
        self.torch, self.orc, self.parse = torch, orc, parse
        docs = documents()
        self.doc = Doc(orc, docs["twitter_like"])
        self.nd = Doc(orc, docs["amazon_ndjson"])
        self.tok_in = so.Late(self.doc.a[self.doc.idx], pad=16)
        self.parsers = {}
        ec, tape, sbuf = parse(self.doc.a)
        dc, dtape, dsbuf = parse(self.doc.decoy)
        assert ec == dc == 0
        self.doc_tape, self.doc_sbuf = tape, sbuf
        table = np.zeros(2, capi.DOC_SPAN)
        table[1] = (self.doc.n, self.doc.L, len(tape), len(sbuf))
        self.twitter = LateTapes((tape, sbuf, table), (dtape, dsbuf, table))
        self.nd_tapes = stream_tapes(parse, self.nd.a, self.nd.idx)
        self.amazon = LateTapes(self.nd_tapes, stream_tapes(parse, self.nd.decoy, self.nd.idx))
        A = self.amazon.T
        whole = test_gpu_query.model(A, [b""])
        self.records = (whole[0][0], whole[1][0])  # the root cell of every amazon record
        self.users = self.matches(self.twitter.T, USERS)
        self.hashtags = self.matches(self.twitter.T, HASHTAGS)
        assert len(self.users[0]) == len(self.hashtags[0]) > 500 and (self.users[0] == ord("{")).all() and (self.hashtags[0] == ord("[")).all()

    @staticmethod
    def matches(T, path):
        status, offsets, tags, values = test_gpu_paths.as_column(test_gpu_paths.model_cells(T, [path]))
        return tags, values

    def parser(self, pipeline="auto"):
        if pipeline not in self.parsers:
            self.parsers[pipeline] = capi.DomParserImplementation(CAP)
            self.parsers[pipeline].set_pipeline(pipeline)
        return self.parsers[pipeline]

    def close(self):
        for p in self.parsers.values():
            p.close()


@pytest.fixture(scope="module")
def world():
    build.build_sjgpu()
    orc = checkers.Oracle()
    parse = lambda d, md=1024: orc.dom_parse(d, md)  # noqa: E731
    if checkers.have_reference_lib():
        ref = checkers.Reference()
        impl = ref.best_impl()
        if impl:
            parse = lambda d, md=1024: ref.dom_parse(impl, d, md)  # noqa: E731
    w = World(orc, parse)
    yield w
    w.close()


@pytest.fixture(scope="module")
def delay():
    """the copy pass, timed once for the module (the only one that uses it)"""
    d = so.Delay()
    print(f"DELAY one copy pass of {so.SCRATCH_BYTES >> 20} MiB: {d.pass_ms:.3f} ms")
    return d


@pytest.fixture(scope="module")
def side(delay):
    return so.concurrent_stream(delay)


def roots_in(roots):
    """a row of root cells as late inputs (cells of containers and strings hold structure only: the decoy document's are the same)"""
    return so.Late(np.ascontiguousarray(roots[1], np.uint64), pad=1), so.Late(np.ascontiguousarray(roots[0], np.uint8), pad=1)


# ---- a. the table: name of the method -> the cases that probe it -------------------------------------------------------------------------------------
def _stage1(W, tokens, name):
    import torch
    D, cases = W.doc, []
    for pipeline in ("split", "fused"):
        p = W.parser(pipeline)
        idx = so.poisoned(D.n + 3, torch.int32)
        tok = so.poisoned(D.n + 3, torch.uint8)

        def enqueue(st, p=p, idx=idx, tok=tok, pipeline=pipeline):
            if tokens:
                assert p.stage1_tokens_device(D.buf.ptr, D.L, idx.data_ptr(), D.n + 3, tok.data_ptr(), D.n + 3, st) == 0, "stage1_tokens_device refused"
            else:
                assert p.stage1_device(D.buf.ptr, D.L, idx.data_ptr(), D.n + 3, st) == 0, "stage1_device refused"
            assert p.last_pipeline() == pipeline, (p.last_pipeline(), pipeline)

        def check(ret, kept, note):
            assert ret[:2] == (D.n, D.flags), (ret, D.n, note)
            assert np.array_equal(kept[0], D.list), f"the structural list {note}"
            if tokens:
                assert np.array_equal(kept[1][: D.n], D.a[D.idx]), f"the token bytes {note}"
        cases.append(so.Case(f"{name}[{pipeline}]", [D.buf], [idx, tok] if tokens else [idx], enqueue, check, finish=lambda st, ret, p=p: p.result(st), only_enqueues=True))
    return cases


def _minified(W, p, name, inputs, dst, enqueue, want):
    def check(ret, kept, note):
        _, flags, out_len = ret
        assert (flags, out_len) == (0, len(want)), (ret, len(want), note)
        assert np.array_equal(kept[0][:out_len], want), f"the minified bytes {note}"
        assert (kept[0][out_len:] == so.POISON).all(), f"bytes behind dst + out_len {note}"
    return so.Case(name, inputs, [dst], enqueue, check, finish=lambda st, ret: p.result(st), only_enqueues=True)


def minify_device(W):
    import torch
    D, cases = W.doc, []
    err, want = W.orc.minify(D.a)
    assert err == 0
    for pipeline in ("split", "fused"):
        p = W.parser(pipeline)
        dst = so.poisoned(D.L, torch.uint8)

        def enqueue(st, p=p, dst=dst, pipeline=pipeline):
            assert p.minify_device(D.buf.ptr, D.L, dst.data_ptr(), st) == 0, "minify_device refused"
            assert p.last_pipeline() == pipeline, (p.last_pipeline(), pipeline)
        cases.append(_minified(W, p, f"minify_device[{pipeline}]", [D.buf], dst, enqueue, want))
    return cases


def _one_bit(W, name, spoil, enqueue_of, bit_of, want_of):
    """a call that answers with one bit about ANY bytes: the real input against a decoy with the other answer, both ways round"""
    D, p, cases = W.doc, W.parser(), []
    for real, decoy, which in ((D.a, spoil(D.decoy), "the document"), (spoil(D.a), D.decoy, "the spoilt document")):
        buf = so.Late(real, decoy, pad=64)
        want = want_of(real)
        assert want != want_of(decoy)

        def check(ret, kept, note, want=want):
            assert bit_of(ret) == want, (ret, want, note)
        cases.append(so.Case(f"{name}[{which}]", [buf], [], lambda st, buf=buf: enqueue_of(p, buf, st), check, finish=lambda st, ret: p.result(st), only_enqueues=True))
    return cases


def validate_utf8_device(W):
    def enqueue(p, buf, st):
        assert p.validate_utf8_device(buf.ptr, W.doc.L, st) == 0, "validate_utf8_device refused"
    return _one_bit(W, "validate_utf8_device", so.break_utf8, enqueue, lambda ret: not ret[1] & capi.F_UTF8_ERROR, W.orc.validate_utf8)


def string_parity_device(W):
    """(the method of capi waits: it fetches the bit with result(); here the C entry point is called, the gate looked at, and the bit fetched as the method does)"""
    def enqueue(p, buf, st):
        assert p.L.sjgpu_string_parity_device(p.h, buf.ptr, W.doc.L, st or None) == 0, "sjgpu_string_parity_device refused"
    return _one_bit(W, "string_parity_device", so.flip_parity, enqueue, lambda ret: ret[0] & 1, lambda a: W.orc.scan(a)[1] & capi.F_UNCLOSED_STRING)


def shard_of(orc, a):
    """the second shard of a document, cut inside a string (host only) -> (cut, in_string, the oracle's list of the shard, the oracle's minified bytes of it)"""
    a = np.ascontiguousarray(a, np.uint8)
    inside, _ = so.string_masks(a)
    run = np.convolve(inside.astype(np.int32), np.ones(32, np.int32), "same")
    target = len(a) // 2 + int(np.argmax(run[len(a) // 2:] == 32))  # the middle of 32 bytes of text
    cut = capi.clean_cut(a, target)
    in_string = orc.scan(a[:cut])[1] & capi.F_UNCLOSED_STRING
    assert 0 < cut < len(a) and in_string == 1, (cut, in_string)
    L = len(a) - cut
    whole = np.concatenate([np.frombuffer(HEAD, np.uint8), a[cut:]])
    idx, flags = orc.scan(whole)
    err, out = orc.minify(whole)
    assert flags == 0 and err == 0
    return cut, 1, np.concatenate([idx[idx >= 16] - 16, np.array([L, L, 0], np.uint32)]).astype(np.uint32), out[16:]


def _shard(W):
    """-> (the shard's bytes as a late input, its length, in_string, the oracle's list, the oracle's minified bytes)"""
    if not hasattr(W, "shard"):
        D = W.doc
        cut, in_string, want_list, want_min = shard_of(W.orc, D.a)
        W.shard = (so.Late(D.a[cut:], D.decoy[cut:], pad=64), D.L - cut, in_string, want_list, want_min)
    return W.shard


def stage1_shard_device(W):
    import torch
    buf, L, in_string, want, _ = _shard(W)
    p, n = W.parser("fused"), len(want) - 3
    idx = so.poisoned(n + 3, torch.int32)

    def check(ret, kept, note):
        assert ret[:2] == (n, 0), (ret, n, note)
        assert np.array_equal(kept[0], want), f"the shard's list {note}"
    return [so.Case("stage1_shard_device", [buf], [idx], lambda st: p.stage1_shard_device(buf.ptr, L, in_string, idx.data_ptr(), n + 3, st), check,
                    finish=lambda st, ret: p.result(st), only_enqueues=True)]


def minify_shard_device(W):
    import torch
    buf, L, in_string, _, want = _shard(W)
    p = W.parser("split")
    dst = so.poisoned(L, torch.uint8)
    return [_minified(W, p, "minify_shard_device", [buf], dst, lambda st: p.minify_shard_device(buf.ptr, L, in_string, dst.data_ptr(), st), want)]


def range_handoff(orc, a):
    """what the first range hands to the second, from the oracle (host only) -> (in_string bits, structurals in front, minified bytes in front, all minified bytes)"""
    a = np.ascontiguousarray(a, np.uint8)
    idx, flags = orc.scan(a[:RANGE])
    in_string = flags & capi.F_UNCLOSED_STRING
    _, escaped = so.string_masks(a)
    assert not escaped[RANGE] and a[RANGE - 1] != 0x5C, "the document's byte at 1 MiB is escaped: this cut needs SJGPU_F_RANGE_CARRY too"
    tail = np.concatenate([np.frombuffer(HEAD, np.uint8), a[RANGE:]]) if in_string else a[RANGE:]
    err, out = orc.minify(tail)
    whole = orc.minify(a)[1]
    assert err == 0
    return in_string, len(idx), len(whole) - (len(out) - (16 if in_string else 0)), whole


def _range_handoff(W):
    return range_handoff(W.orc, W.doc.a)


def stage1_range_device(W):
    """two ranges back to back, the second with the hand-off the oracle gives: no result is fetched between them"""
    import torch
    D, p = W.doc, W.parser("fused")
    in_string, n_before, _, _ = _range_handoff(W)
    idx = so.poisoned(D.n + 3, torch.int32)

    def enqueue(st):
        p.stage1_range_device(D.buf.ptr, 0, RANGE, 1, 0, 0, idx.data_ptr(), D.n + 3, st)
        p.stage1_range_device(D.buf.ptr, RANGE, D.L, 0, in_string, n_before, idx.data_ptr(), D.n + 3, st)

    def check(ret, kept, note):
        assert ret[:2] == (D.n, 0), (ret, D.n, note)
        assert np.array_equal(kept[0], D.list), f"the list of both ranges {note}"
    return [so.Case("stage1_range_device", [D.buf], [idx], enqueue, check, finish=lambda st, ret: p.result(st), only_enqueues=True)]


def minify_range_device(W):
    import torch
    D, p = W.doc, W.parser("split")
    in_string, _, out_before, whole = _range_handoff(W)
    dst = so.poisoned(D.L, torch.uint8)

    def enqueue(st):
        p.minify_range_device(D.buf.ptr, 0, RANGE, 1, 0, 0, dst.data_ptr(), st)
        p.minify_range_device(D.buf.ptr, RANGE, D.L, 0, in_string, out_before, dst.data_ptr(), st)
    return [_minified(W, p, "minify_range_device", [D.buf], dst, enqueue, whole)]


def stage1_finish_device(W):
    """streaming_final over the records with the last one cut off behind its opening bracket: the list shrinks to the complete documents, in place"""
    N, p = W.nd, W.parser()
    mode = checkers.MODES["streaming_final"]
    cut = line_begins(N.a)[-1] + 1
    a = N.a[:cut]
    raw, flags = W.orc.scan(a)
    assert flags == 0
    want = checkers.observable(a, mode, *W.orc.stage1(a, mode))
    assert len(want) == 3 and want[0] == 0 and want[1] < len(raw), want[:2]
    buf = so.Late(a, N.decoy[:cut], pad=64)
    idx = so.Late(np.concatenate([raw, np.array([cut, cut, 0], np.uint32)]).astype(np.uint32))

    def check(ret, kept, note):
        err, n, _ = ret
        assert (err, n) == want[:2], (ret, want[:2], note)
        assert tuple(kept[0][: n + 3].tolist()) == want[2], f"the list finish() leaves {note}"
    return [so.Case("stage1_finish_device", [buf], [], lambda st: p.stage1_finish_device(buf.ptr, cut, mode, idx.ptr, len(raw), flags, st), check, inouts=[idx])]


def _depths(W):
    c = W.doc.a[W.doc.idx]
    delta = np.isin(c, [ord("{"), ord("[")]).astype(np.int64) - np.isin(c, [ord("}"), ord("]")]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(delta)]).astype(np.uint32)


def depth_scan_device(W):
    import torch
    D, p, want = W.doc, W.parser(), _depths(W)
    depth = so.poisoned(D.n + 1, torch.int32)

    def check(ret, kept, note):
        assert np.array_equal(kept[0], want), f"the depths {note}"
    return [so.Case("depth_scan_device", [D.buf, D.idx_in], [depth], lambda st: p.depth_scan_device(D.buf.ptr, D.idx_in.ptr, D.n, depth.data_ptr(), st), check, only_enqueues=True)]


def depth_scan_tokens_device(W):
    import torch
    D, p, want = W.doc, W.parser(), _depths(W)
    depth = so.poisoned(D.n + 1, torch.int32)

    def check(ret, kept, note):
        assert np.array_equal(kept[0], want), f"the depths {note}"
    return [so.Case("depth_scan_tokens_device", [W.tok_in], [depth], lambda st: p.depth_scan_tokens_device(W.tok_in.ptr, D.n, depth.data_ptr(), st), check, only_enqueues=True)]


def parse_strings_device(W):
    import torch
    D, p = W.doc, W.parser()
    err, wbytes, woff, wstrings, wbad = W.orc.string_buffer(D.a, D.list[: D.n + 1], D.n)
    assert err == 0 and wbad == checkers.NO_STRING
    want_off = np.where(woff != checkers.NO_STRING, woff, np.uint32(len(wbytes))).astype(np.uint32)
    want_off = np.concatenate([np.minimum.accumulate(want_off[::-1])[::-1], np.array([len(wbytes)], np.uint32)]).astype(np.uint32)
    sbuf, off = so.poisoned(len(wbytes), torch.uint8), so.poisoned(D.n + 1, torch.int32)

    def check(ret, kept, note):
        assert ret == (0, len(wbytes), wstrings, checkers.NO_STRING), (ret, len(wbytes), wstrings, note)
        assert np.array_equal(kept[0], wbytes), f"the string buffer {note}"
        assert np.array_equal(kept[1], want_off), f"the record offsets {note}"
    return [so.Case("parse_strings_device", [D.buf, D.idx_in], [sbuf, off],
                    lambda st: p.parse_strings_device(D.buf.ptr, D.L, D.idx_in.ptr, D.n, sbuf.data_ptr(), len(wbytes), off.data_ptr(), False, st), check)]


def match_keys_device(W):
    import torch
    D, p = W.doc, W.parser()
    want, wm = W.orc.match_keys(D.a, D.list[: D.n + 1], D.n, KEY_NAMES)
    assert wm > 10000 and W.orc.match_keys(D.decoy, D.list[: D.n + 1], D.n, KEY_NAMES)[1] != wm  # (the decoy's keys are other names)
    out = so.poisoned(D.n, torch.int32)

    def check(ret, kept, note):
        assert ret == wm, (ret, wm, note)
        assert np.array_equal(kept[0], want), f"the matches {note}"
    return [so.Case("match_keys_device", [D.buf, D.idx_in], [out], lambda st: p.match_keys_device(D.buf.ptr, D.L, D.idx_in.ptr, D.n, KEY_NAMES, out.data_ptr(), st), check)]


def stage2_device(W):
    import torch
    D, p, cases = W.doc, W.parser(), []
    for tokens in (False, True):
        tape, sbuf = so.poisoned(len(W.doc_tape), torch.int64), so.poisoned(len(W.doc_sbuf), torch.uint8)

        def enqueue(st, tape=tape, sbuf=sbuf, tokens=tokens):
            return p.stage2_device(D.buf.ptr, D.L, D.idx_in.ptr, D.n, tape.data_ptr(), len(W.doc_tape), sbuf.data_ptr(), len(W.doc_sbuf), stream=st,
                                   tok_ptr=W.tok_in.ptr if tokens else 0)

        def check(ret, kept, note):
            assert ret == (0, len(W.doc_tape), len(W.doc_sbuf)), (ret, len(W.doc_tape), len(W.doc_sbuf), note)
            assert np.array_equal(kept[0], W.doc_tape), f"the tape {note}"
            assert np.array_equal(kept[1], W.doc_sbuf), f"the string buffer {note}"
        cases.append(so.Case("stage2_device" + ("[tok_ptr]" if tokens else ""), [D.buf, D.idx_in] + ([W.tok_in] if tokens else []), [tape, sbuf], enqueue, check))
    return cases


def _stage2_many(W, p, N, want, name="stage2_many_device"):
    import torch
    wtape, wsbuf, wtable = want
    docs = len(wtable) - 1
    tape, sbuf, table = so.poisoned(len(wtape), torch.int64), so.poisoned(len(wsbuf), torch.uint8), so.poisoned((docs + 1) * 4, torch.int32)

    def enqueue(st):
        return p.stage2_many_device(N.buf.ptr, N.L, N.idx_in.ptr, N.n, tape.data_ptr(), len(wtape), sbuf.data_ptr(), len(wsbuf), table.data_ptr(), docs + 1, stream=st)

    def check(ret, kept, note):
        assert ret == (0, docs, len(wtape), len(wsbuf)), (ret, docs, len(wtape), len(wsbuf), note)
        assert np.array_equal(kept[0], wtape), f"the tapes {note}"
        assert np.array_equal(kept[1], wsbuf), f"the string records {note}"
        assert np.array_equal(kept[2], wtable.view(np.uint32)), f"the document table {note}"
    return so.Case(name, [N.buf, N.idx_in], [tape, sbuf, table], enqueue, check)


def stage2_many_device(W):
    return [_stage2_many(W, W.parser(), W.nd, W.nd_tapes)]


def _columns_case(name, inputs, K, rows, call, want):
    """a call that leaves K * rows cells: values and tags"""
    import torch
    values, tags = so.poisoned(K * rows, torch.int64), so.poisoned(K * rows, torch.uint8)

    def check(ret, kept, note):
        assert ret == 0, (ret, note)
        test_gpu_query.assert_columns((kept[1].reshape(K, rows), kept[0].reshape(K, rows)), want, f"{note} ")
    return so.Case(name, inputs, [values, tags], lambda st: call(values.data_ptr(), tags.data_ptr(), st), check)


def at_pointers_device(W, pointers=POINTERS, name="at_pointers_device"):
    A, p = W.amazon, W.parser()
    want = test_gpu_query.model(A.T, pointers)
    assert (want[0] == ord("d")).sum() > 1000 and (want[0] == ord("l")).sum() > 1000  # the ratings and the reviews: numbers, other ones in the decoy
    return [_columns_case(name, A.inputs, len(pointers), A.T.docs, lambda v, t, st: p.at_pointers_device(*A.args(), pointers, v, t, st), want)]


def gather_strings_device(W):
    import torch
    A, p = W.amazon, W.parser()
    tags, values = (x[0] for x in test_gpu_query.model(A.T, [b"/2"]))
    strings = [pointer_model.string_of(A.T.sbuf, int(v)) if t == ord('"') else b"" for t, v in zip(tags, values)]
    total = sum(len(s) for s in strings)
    want_offsets = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint32)
    assert total > 50000
    row_values, row_tags = roots_in((tags, values))
    offsets, chars = so.poisoned(A.T.docs + 1, torch.int32), so.poisoned(total, torch.uint8)

    def check(ret, kept, note):
        assert ret == (0, total), (ret, total, note)
        assert np.array_equal(kept[0], want_offsets), f"the offsets {note}"
        assert kept[1].tobytes() == b"".join(strings), f"the characters {note}"
    return [so.Case("gather_strings_device", [A.sbuf, row_values, row_tags], [offsets, chars],
                    lambda st: p.gather_strings_device(A.sbuf.ptr, len(A.T.sbuf), row_values.ptr, row_tags.ptr, A.T.docs, offsets.data_ptr(), chars.data_ptr(), total, st), check)]


def _ragged_case(name, inputs, cells, want, call):
    """a call that leaves a ragged column: offsets (cells + 1), status (cells), and as many values and tags as the model has matches"""
    import torch
    wstatus, woffsets, wtags, wvalues = want
    cap = len(wtags)
    assert cap > 1000
    offsets, status = so.poisoned(cells + 1, torch.int32), so.poisoned(cells, torch.uint8)
    values, tags = so.poisoned(cap, torch.int64), so.poisoned(cap, torch.uint8)

    def check(ret, kept, note):
        assert ret == (0, cap), (ret, cap, note)
        path_cases.assert_column((kept[1].reshape(wstatus.shape), kept[0], kept[3], kept[2]), want, f"{note} ")
    return so.Case(name, inputs, [offsets, status, values, tags], lambda st: call(offsets.data_ptr(), status.data_ptr(), values.data_ptr(), tags.data_ptr(), cap, st), check)


def _at_paths(W, method):
    A, p = W.amazon, W.parser()
    want = test_gpu_paths.as_column(test_gpu_paths.model_cells(A.T, PATHS))
    return [_ragged_case(method, A.inputs, len(PATHS) * A.T.docs, want, lambda o, s, v, t, cap, st: getattr(p, method)(*A.args(), PATHS, o, s, v, t, cap, st))]


def at_pointers_from_cells_device(W):
    A, p = W.amazon, W.parser()
    pointers = [b"/5", b"/7", b"/1", b"/9"]
    rv, rt = roots_in(W.records)
    want = test_gpu_rows.model(A.T, W.records, pointers)
    rows = len(W.records[0])
    return [_columns_case("at_pointers_from_cells_device", A.inputs + [rv, rt], len(pointers), rows,
                          lambda v, t, st: p.at_pointers_from_cells_device(*A.args(), rv.ptr, rt.ptr, rows, pointers, v, t, st), want)]


def at_paths_from_cells_device(W):
    A, p = W.amazon, W.parser()
    paths = [b"$[*]", b"$[5]"]
    rv, rt = roots_in(W.records)
    rows = len(W.records[0])
    want = test_gpu_lists.model(A.T, W.records, paths)
    return [_ragged_case("at_paths_from_cells_device", A.inputs + [rv, rt], len(paths) * rows, want,
                         lambda o, s, v, t, cap, st: p.at_paths_from_cells_device(*A.args(), rv.ptr, rt.ptr, rows, paths, o, s, v, t, cap, st))]


def object_fields_from_cells_device(W):
    """the users of the twitter-like document: their ids and counts are numbers, and the decoy's are others"""
    import torch
    X, p = W.twitter, W.parser()
    rows = len(W.users[0])
    rv, rt = roots_in(W.users)
    want = test_gpu_fields.model(X.T, W.users)[0]
    cap = len(want[4])
    assert cap > 2000
    offsets, status = so.poisoned(rows + 1, torch.int32), so.poisoned(rows, torch.uint8)
    words, tags = [so.poisoned(cap, torch.int64) for _ in range(2)], [so.poisoned(cap, torch.uint8) for _ in range(2)]

    def enqueue(st):
        return p.object_fields_from_cells_device(*X.args(), rv.ptr, rt.ptr, rows, offsets.data_ptr(), status.data_ptr(), words[0].data_ptr(), tags[0].data_ptr(),
                                                 words[1].data_ptr(), tags[1].data_ptr(), cap, st)

    def check(ret, kept, note):
        assert ret == (0, cap), (ret, cap, note)
        fields_model.assert_columns((kept[1], kept[0], kept[4], kept[2], kept[5], kept[3]), want, f"{note} ")
    return [so.Case("object_fields_from_cells_device", X.inputs + [rv, rt], [offsets, status] + words + tags, enqueue, check)]


def _sizes_case(W, name="cell_sizes_device"):
    import torch
    X, p = W.twitter, W.parser()
    rows = len(W.hashtags[0])
    rv, rt = roots_in(W.hashtags)
    want = fields_model.sizes(fields_model.Stream(X.T.tape, X.T.sbuf, X.T.table), W.hashtags)
    assert len(set(want[0].tolist())) >= 3 and not want[1].any()
    size, code = so.poisoned(rows, torch.int32), so.poisoned(rows, torch.uint8)

    def check(ret, kept, note):
        assert ret == 0, (ret, note)
        assert np.array_equal(kept[0], want[0]) and np.array_equal(kept[1], want[1]), f"the sizes {note}"
    return so.Case(name, [X.tape, X.table, rv, rt], [size, code],
                   lambda st: p.cell_sizes_device(X.tape.ptr, len(X.T.tape), X.table.ptr, X.T.docs, rv.ptr, rt.ptr, rows, size.data_ptr(), code.data_ptr(), st), check)


N_CELLS, K_CELLS = 8449, 3


def _cells(W):
    if not hasattr(W, "cells"):
        tags, values = random_cells(np.random.default_rng(95), N_CELLS, K_CELLS)
        decoy = so.decoy_cells(values)
        assert not np.array_equal(cast_model.kinds(tags, values), cast_model.kinds(tags, decoy))
        W.cells = (tags, values, so.Late(values, decoy), so.Late(tags))
    return W.cells


def cast_cells_device(W):
    import torch
    p, cases = W.parser(), []
    tags, values, d_values, d_tags = _cells(W)
    W_words = (N_CELLS + 63) // 64
    for in_place in (False, True):
        getters = cycled(K_CELLS, 2 if in_place else 0)
        want = cast_model.cast(tags, values, getters)
        value_out, code_out = so.poisoned(K_CELLS * N_CELLS, torch.int64), so.poisoned(K_CELLS * N_CELLS, torch.uint8)
        valid, counts = so.poisoned(K_CELLS * W_words, torch.int64), so.poisoned(K_CELLS * 4, torch.int32)
        outs = [valid, counts] if in_place else [value_out, code_out, valid, counts]

        def enqueue(st, getters=getters, in_place=in_place, value_out=value_out, code_out=code_out, valid=valid, counts=counts):
            return p.cast_cells_device(d_values.ptr, d_tags.ptr, N_CELLS, getters, d_values.ptr if in_place else value_out.data_ptr(),
                                       d_tags.ptr if in_place else code_out.data_ptr(), valid.data_ptr(), counts.data_ptr(), st)

        def check(ret, kept, note, want=want, in_place=in_place):
            assert ret == 0, (ret, note)
            got = (kept[2], kept[3], kept[0], kept[1]) if in_place else kept  # (the inouts are kept behind the outputs)
            for mine, w, what in zip(got, want, ("value_out", "code_out", "valid_out", "counts")):
                assert np.array_equal(mine.reshape(w.shape), w), f"{what} {note}"
        cases.append(so.Case("cast_cells_device" + ("[in place]" if in_place else ""), [] if in_place else [d_values, d_tags], outs, enqueue, check, only_enqueues=True,
                             inouts=[d_values, d_tags] if in_place else []))
    return cases


def cell_kinds_device(W):
    import torch
    p = W.parser()
    tags, values, d_values, d_tags = _cells(W)
    want = cast_model.kinds(tags, values)
    kinds = so.poisoned(K_CELLS * 16, torch.int32)

    def check(ret, kept, note):
        assert ret == 0, (ret, note)
        assert np.array_equal(kept[0].reshape(K_CELLS, 16), want), f"the census {note}"
    return [so.Case("cell_kinds_device", [d_values, d_tags], [kinds], lambda st: p.cell_kinds_device(d_values.ptr, d_tags.ptr, N_CELLS, K_CELLS, kinds.data_ptr(), st), check,
                    only_enqueues=True)]


TABLE = {
    "stage1_device": lambda W: _stage1(W, False, "stage1_device"),
    "stage1_tokens_device": lambda W: _stage1(W, True, "stage1_tokens_device"),
    "minify_device": minify_device,
    "validate_utf8_device": validate_utf8_device,
    "string_parity_device": string_parity_device,
    "stage1_shard_device": stage1_shard_device,
    "minify_shard_device": minify_shard_device,
    "stage1_range_device": stage1_range_device,
    "minify_range_device": minify_range_device,
    "stage1_finish_device": stage1_finish_device,
    "depth_scan_device": depth_scan_device,
    "depth_scan_tokens_device": depth_scan_tokens_device,
    "parse_strings_device": parse_strings_device,
    "match_keys_device": match_keys_device,
    "stage2_device": stage2_device,
    "stage2_many_device": stage2_many_device,
    "at_pointers_device": at_pointers_device,
    "gather_strings_device": gather_strings_device,
    "at_paths_device": lambda W: _at_paths(W, "at_paths_device"),
    "at_paths_wide_device": lambda W: _at_paths(W, "at_paths_wide_device"),
    "at_pointers_from_cells_device": at_pointers_from_cells_device,
    "at_paths_from_cells_device": at_paths_from_cells_device,
    "object_fields_from_cells_device": object_fields_from_cells_device,
    "cell_sizes_device": lambda W: [_sizes_case(W)],
    "cast_cells_device": cast_cells_device,
    "cell_kinds_device": cell_kinds_device,
}


def probe(case, side, delay):
    t0 = time.perf_counter()
    ret, kept, note = so.late_call(case, side, delay)
    case.check(ret, kept, note)
    print(f"CASE {case.name}: {time.perf_counter() - t0:.2f} s {note}")


@pytest.mark.parametrize("entry", list(TABLE))
def test_entry_point_with_late_inputs(world, side, delay, entry):
    for case in TABLE[entry](world):
        probe(case, side, delay)


# ---- b. calls with an enqueued tail, back to back ----------------------------------------------------------------------------------------------------
def test_enqueued_tails_back_to_back(world, side, delay):
    """Two sjgpu_at_pointers_device calls with different pointers, then sjgpu_cell_sizes_device behind sjgpu_at_pointers_from_cells_device: one context, one
    side stream, no wait of the test's between them.  Each call's compiled pointers go up through the context's one program block while the walk of the
    call before it is only enqueued (ev_query guards the block)."""
    W = world
    first, = at_pointers_device(W, POINTERS, "at_pointers_device, first")
    second, = at_pointers_device(W, [b"/7", b"/1", b"/8", b"/5", b"/2/x", b"", b"/3"], "at_pointers_device, second")

    def pair(name, a, b):
        def check(ret, kept, note):
            a.check(ret[0], kept[: len(a.outputs)], note)
            b.check(ret[1], kept[len(a.outputs):], note)
        inputs = a.inputs + [i for i in b.inputs if i not in a.inputs]
        return so.Case(name, inputs, a.outputs + b.outputs, lambda st: (a.enqueue(st), b.enqueue(st)), check)
    probe(pair("at_pointers_device twice", first, second), side, delay)
    X, p = W.twitter, W.parser()
    pointers = [b"/id", b"/followers_count", b"/entities/hashtags", b"/name"]
    rv, rt = roots_in(W.users)
    rows = len(W.users[0])
    rooted = _columns_case("at_pointers_from_cells_device", X.inputs + [rv, rt], len(pointers), rows,
                           lambda v, t, st: p.at_pointers_from_cells_device(*X.args(), rv.ptr, rt.ptr, rows, pointers, v, t, st), test_gpu_rows.model(X.T, W.users, pointers))
    probe(pair("cell_sizes_device behind at_pointers_from_cells_device", rooted, _sizes_case(W)), side, delay)


# ---- c. one context moving between streams -----------------------------------------------------------------------------------------------------------
def test_one_context_moves_between_streams(world, side, delay):
    """Waited calls on side stream A, side stream B, the NULL stream and A again: the single-pass stage 1 (it finds its workspace clean because the call before
    it, on whatever stream, left it so) and stage 2 behind it, one context.  On the side streams the pair goes through late_call: the NULL stream is busy,
    the document arrives late, list, tape and strings are consumed on the stream.  On the NULL stream the calls are made plainly and waited for."""
    import torch
    W, D = world, world.doc
    p = capi.DomParserImplementation(CAP)
    p.set_pipeline("fused")
    idx, tape, sbuf = so.poisoned(D.n + 3, torch.int32), so.poisoned(len(W.doc_tape), torch.int64), so.poisoned(len(W.doc_sbuf), torch.uint8)
    other = so.concurrent_stream(delay, beside=[side])

    def enqueue(st):
        assert p.stage1_device(D.buf.ptr, D.L, idx.data_ptr(), D.n + 3, st) == 0, "stage1_device refused"
        assert p.last_pipeline() == "fused", p.last_pipeline()
        scan = p.result(st)
        return scan, p.stage2_device(D.buf.ptr, D.L, idx.data_ptr(), D.n, tape.data_ptr(), len(W.doc_tape), sbuf.data_ptr(), len(W.doc_sbuf), stream=st)

    def check(ret, kept, note):
        assert ret[0][:2] == (D.n, 0) and ret[1] == (0, len(W.doc_tape), len(W.doc_sbuf)), (ret, D.n, len(W.doc_tape), len(W.doc_sbuf), note)
        assert np.array_equal(kept[0], D.list), f"the structural list {note}"
        assert np.array_equal(kept[1], W.doc_tape) and np.array_equal(kept[2], W.doc_sbuf), f"tape and string buffer {note}"
    for k, s in enumerate((side, other, None, side)):
        case = so.Case(f"call {k}: stage1_device + stage2_device on {'the NULL stream' if s is None else 'side stream ' + 'AB'[s is other]}", [D.buf], [idx, tape, sbuf], enqueue, check)
        if s is not None:
            probe(case, s, delay)
            continue
        note = f"{case.name} [no delay: copy pass {delay.pass_ms:.3f} ms, 0 passes]"
        D.buf.live.copy_(D.buf.real)
        for o in case.outputs:
            so.poison(o)
        ret = so.noted(note, enqueue, 0)
        torch.cuda.synchronize()
        check(ret, [so.host(o) for o in case.outputs], note)
        D.buf.live.copy_(D.buf.decoy)
        torch.cuda.synchronize()
    # A, B and A again with no call on the NULL stream between them (late_call warms up there): nothing allocates any more, the NULL stream is busy throughout
    count = int(so.MAX_MS / delay.pass_ms)
    note = f"[A, B, A back to back; copy pass {delay.pass_ms:.3f} ms, {count} passes on the NULL stream]"
    null_done, consumed = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kept = [[torch.empty_like(o) for o in (idx, tape, sbuf)] for _ in range(3)]
    for o in (idx, tape, sbuf):
        so.poison(o)
    torch.cuda.synchronize()
    delay.enqueue(torch.cuda.default_stream(), count, 0)
    null_done.record(torch.cuda.default_stream())
    rets = []
    for k, s in enumerate((side, other, side)):
        with torch.cuda.stream(s):
            D.buf.live.copy_(D.buf.real, non_blocking=True)
            rets.append(so.noted(note, enqueue, s.cuda_stream))
            for dst, o in zip(kept[k], (idx, tape, sbuf)):
                dst.copy_(o, non_blocking=True)
                so.poison(o)
            D.buf.live.copy_(D.buf.decoy, non_blocking=True)
            consumed.record(s)
        s.synchronize()  # (the next stream's first copy must not overtake this stream's last)
    torch.cuda.synchronize()
    assert consumed.elapsed_time(null_done) > 0, f"the probe was NOT CONCLUSIVE: the NULL stream's delay ended before the last outputs were consumed {note}"
    for k in range(3):
        check(rets[k], [so.host(x) for x in kept[k]], f"call {k} {note}")
    p.close()


# ---- d. two contexts, two streams, one host thread ---------------------------------------------------------------------------------------------------
def test_two_contexts_on_two_streams(world, side, delay):
    """A's call on s1 and B's on s2 (distinct streams that run beside each other and beside the NULL stream), both with late inputs and different documents,
    both enqueued before either outcome is fetched: stage 1 (fetched with result()), then one sjgpu_stage2_many_device per context.  Neither sees the
    other's document.  so.late_calls sets the delays, the gates and both NOT CONCLUSIVE checks as for one call."""
    import torch
    W = world
    streams = [side, so.concurrent_stream(delay, beside=[side])]
    assert streams[0].cuda_stream != streams[1].cuda_stream, f"one stream twice [copy pass {delay.pass_ms:.3f} ms]"
    ctxs = [capi.DomParserImplementation(CAP), capi.DomParserImplementation(CAP)]
    docs = [W.doc, Doc(W.orc, documents()["large_random"])]
    assert not np.array_equal(docs[0].list, docs[1].list)
    cases = []
    for k, (d, p) in enumerate(zip(docs, ctxs)):
        idx = so.poisoned(d.n + 3, torch.int32)

        def enqueue(st, d=d, p=p, idx=idx):
            assert p.stage1_device(d.buf.ptr, d.L, idx.data_ptr(), d.n + 3, st) == 0, "stage1_device refused"

        def check(ret, kept, note, d=d):
            assert ret[:2] == (d.n, 0), (ret, d.n, note)
            assert np.array_equal(kept[0], d.list), f"the structural list {note}"
        cases.append(so.Case(f"stage1_device, context {k}", [d.buf], [idx], enqueue, check, finish=lambda st, ret, p=p: p.result(st), only_enqueues=True))
    t0 = time.perf_counter()
    for c, (ret, kept, note) in zip(cases, so.late_calls(cases, streams, delay)):
        c.check(ret, kept, note)
    print(f"CASE {cases[0].name} + {cases[1].name}: {time.perf_counter() - t0:.2f} s {note}")
    # one sjgpu_stage2_many_device per context: the call waits for its stream, so the second one is made (and its inputs held back) when the first has returned
    nds = [W.nd, Doc(W.orc, documents()["amazon_ndjson_2"])]
    wants = [W.nd_tapes, stream_tapes(W.parse, nds[1].a, nds[1].idx)]
    cases = [_stage2_many(W, p, n, w, f"stage2_many_device, context {k}") for k, (p, n, w) in enumerate(zip(ctxs, nds, wants))]
    t0 = time.perf_counter()
    for c, (ret, kept, note) in zip(cases, so.late_calls(cases, streams, delay)):
        c.check(ret, kept, note)
    print(f"CASE {cases[0].name} + {cases[1].name}: {time.perf_counter() - t0:.2f} s {note}")
    for p in ctxs:
        p.close()


# ---- e. the *_many calls under `with torch.cuda.stream(s):` ---------------------------------------------------------------------------------------------
def under_a_side_stream(side, delay, call):
    """call() with `side` as torch's current stream and the NULL stream busy for 200 ms (less where the call itself waits for the device: an allocation does)"""
    import torch
    torch.cuda.synchronize()
    count = int(so.MAX_MS / delay.pass_ms)
    delay.enqueue(torch.cuda.default_stream(), count, 0)
    try:
        with torch.cuda.stream(side):
            got = call()
    except AssertionError as e:
        raise AssertionError(f"{e} [a side stream current; copy pass {delay.pass_ms:.3f} ms, {count} passes on the NULL stream]") from e
    finally:
        torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_many_calls_of_twitter_under_a_side_stream(world, side, delay, wide):
    """table_many, lists_many, fields_many and typed_table_many of twitter.json as the modules that own them pin them (Python's json, the models), with a side
    stream current and the NULL stream busy"""
    p = world.parser()
    under_a_side_stream(side, delay, lambda: test_gpu_rows.test_twitter_through_table_many(p, wide))
    under_a_side_stream(side, delay, lambda: test_gpu_lists.test_twitter_through_lists_many(p, wide))
    under_a_side_stream(side, delay, lambda: test_gpu_casts.test_typed_table_of_twitter(p, wide))
    if not wide:  # (the test runs both roads itself)
        under_a_side_stream(side, delay, lambda: test_gpu_fields.test_twitter_users_through_fields_many(p))
    data = open(test_gpu_rows.TWITTER, "rb").read()
    statuses = json.loads(data)["statuses"]
    code, docs, tags, values = under_a_side_stream(side, delay, lambda: p.extract_many(data, [b"/statuses/0/id", b"/statuses/99/user/id", b"/search_metadata/count"]))
    assert (code, docs) == (0, 1) and (tags == ord("l")).all()
    assert values[:, 0].tolist() == [statuses[0]["id"], statuses[99]["user"]["id"], json.loads(data)["search_metadata"]["count"]]
    code, docs, status, offsets, tags, values = under_a_side_stream(side, delay, lambda: p.explode_many(data, [b"$.statuses[*].user.id", b"$.statuses[*].id"], wide=wide))
    assert (code, docs, offsets.tolist()) == (0, 1, [0, 100, 200]) and not status.any() and (tags == ord("l")).all()
    assert values.tolist() == [s["user"]["id"] for s in statuses] + [s["id"] for s in statuses]


@pytest.fixture(scope="module")
def small(world):
    """3 000 small records, the oracle's tapes of them, and the rows of `$.*` from the path model"""
    docs = stream_cases.small_records(np.random.default_rng(121), 3000)
    stream, _ = stream_cases.join(docs, b"\n")
    a = np.frombuffer(stream + b"\n", np.uint8)
    idx, flags = world.orc.scan(a)
    assert flags == 0
    T = test_gpu_query.Tapes(*stream_tapes(world.parse, a, idx))
    row_status, row_offsets, rtags, rvalues = test_gpu_paths.as_column(test_gpu_paths.model_cells(T, [b"$.*"]))
    assert not row_status.any() and len(rtags) > 5000
    return a, T, row_offsets, (rtags, rvalues)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_many_calls_of_small_records_under_a_side_stream(world, side, delay, small, wide):
    """the seven *_many calls over the small records against the models over the oracle's tapes, with a side stream current and the NULL stream busy"""
    p = world.parser()
    a, T, row_offsets, roots = small
    rows = len(roots[0])
    if not wide:
        pointers = test_gpu_query.query_cases.SMALL_RECORD_POINTERS
        code, docs, tags, values = under_a_side_stream(side, delay, lambda: p.extract_many(a, pointers))
        assert (code, docs) == (0, T.docs)
        test_gpu_query.assert_columns((tags, values), test_gpu_query.model(T, pointers), "extract_many: ")
    paths = path_cases.SMALL_RECORD_PATHS
    code, docs, status, offsets, tags, values = under_a_side_stream(side, delay, lambda: p.explode_many(a, paths, wide=wide))
    assert (code, docs) == (0, T.docs)
    path_cases.assert_column((status, offsets, tags, values), test_gpu_paths.as_column(test_gpu_paths.model_cells(T, paths)), "explode_many: ")
    pointers = [b"", b"/1", b"/b/c/1/d", b"/0"]
    want_cells = test_gpu_rows.model(T, roots, pointers)
    code, docs, offsets, tags, values = under_a_side_stream(side, delay, lambda: p.table_many(a, b"$.*", pointers, wide=wide))
    assert (code, docs) == (0, T.docs) and np.array_equal(offsets, row_offsets)
    test_gpu_rows.assert_columns((tags, values), want_cells, "table_many: ")
    lpaths = [b"$[*]", b".b.c[*].d", b"$.*"]
    code, docs, offsets, status, loffsets, tags, values = under_a_side_stream(side, delay, lambda: p.lists_many(a, b"$.*", lpaths, wide=wide))
    assert (code, docs) == (0, T.docs) and np.array_equal(offsets, row_offsets)
    path_cases.assert_column((status, loffsets, tags, values), test_gpu_lists.model(T, roots, lpaths), "lists_many: ")
    code, docs, offsets, status, foffsets, key_offsets, key_chars, tags, values = under_a_side_stream(side, delay, lambda: p.fields_many(a, b"$.*", wide=wide))
    want = test_gpu_fields.model(T, roots)[0]
    assert (code, docs) == (0, T.docs) and np.array_equal(offsets, row_offsets)
    keys = [pointer_model.string_of(T.sbuf, int(v)) for v in want[3]]
    assert np.array_equal(status, want[0]) and np.array_equal(foffsets, want[1]) and np.array_equal(tags, want[4]) and np.array_equal(values, want[5]), "fields_many"
    assert key_chars.tobytes() == b"".join(keys) and key_offsets.tolist() == np.concatenate([[0], np.cumsum([len(k) for k in keys])]).tolist(), "fields_many: the keys"
    code, docs, offsets, columns = under_a_side_stream(side, delay, lambda: p.typed_table_many(a, b"$.*", pointers, wide=wide))
    assert (code, docs) == (0, T.docs) and np.array_equal(offsets, row_offsets)
    kinds = cast_model.kinds(*want_cells)
    getters = cast_model.infer_getters(kinds)
    assert sum(1 for g in getters if g) >= 1
    for k, c in enumerate(columns):
        assert np.array_equal(c["tags"], want_cells[0][k]) and np.array_equal(c["cells"], want_cells[1][k]) and np.array_equal(c["kinds"], kinds[k]), f"typed_table_many: column {k}"
        assert c["getter"] == getters[k], (k, c["getter"], getters[k])
        if not getters[k]:
            continue
        wv, wc, wvalid, wcounts = cast_model.cast(want_cells[0][k: k + 1], want_cells[1][k: k + 1], [getters[k]])
        assert np.array_equal(c["codes"], wc[0]) and np.array_equal(c["counts"], wcounts[0]) and np.array_equal(c["valid"].view(np.uint64), wvalid[0]), f"typed_table_many: column {k}"
        if getters[k] != capi.GET_STRING:
            mine = c["values"].astype(np.uint64) if c["values"].dtype == np.bool_ else c["values"].view(np.uint64)
            assert np.array_equal(mine, wv[0]), f"typed_table_many: the values of column {k}"
        else:
            strings = [pointer_model.string_of(T.sbuf, int(v)) if code == 0 else b"" for v, code in zip(want_cells[1][k], wc[0])]
            assert c["chars"].tobytes() == b"".join(strings) and c["offsets"].tolist() == np.concatenate([[0], np.cumsum([len(s) for s in strings])]).tolist(), k
