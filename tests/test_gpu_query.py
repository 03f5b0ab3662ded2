"""GPU tier (-m gpu): queries over device tapes -- sjgpu_at_pointers_device / sjgpu_gather_strings_device (sjgpu_query.hip, include/sjgpu_query.h) and
capi.extract_many -- against tests/golden/pointers.json (the real reference's at_pointer, cell by cell) and tests/pointer_model.py (pinned against that
fixture and against Python's json on the CPU tier).  The tapes are the device's own: sjgpu_stage2_many_device / sjgpu_stage2_device, which
tests/test_gpu_stream_tape.py pins word for word.  Every output has exactly the contracted size inside a poisoned tensor whose poison is checked."""
import json
import re

import numpy as np
import pytest

import pointer_model
import query_cases
import stream_cases
from simdjson_amd import build, capi
from test_gpu_stream_tape import Resident, many_device

pytestmark = pytest.mark.gpu

CAP = 128 << 20
E_BADARG, E_OVERFLOW = -4, -5
GUARD = 65  # odd: with it the tag rows and the characters begin at odd addresses
P64 = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


class Tapes:
    """tapes, string records and table in device memory at their exact sizes, and their host copies"""

    def __init__(self, tape, sbuf, table):
        import torch
        self.torch = torch
        self.stream = torch.cuda.current_stream().cuda_stream
        self.tape, self.sbuf, self.table = np.ascontiguousarray(tape, np.uint64), np.ascontiguousarray(sbuf, np.uint8), table
        self.docs = len(table) - 1
        self.d_tape = torch.from_numpy(self.tape.view(np.int64)).cuda()
        self.d_sbuf = torch.from_numpy(np.concatenate([self.sbuf, np.full(16, 0x5A, np.uint8)])).cuda()  # (never empty: an address to pass; what lies behind is no slack)
        self.d_table = torch.from_numpy(np.ascontiguousarray(table).view(np.int32)).cuda()

    @classmethod
    def of_stream(cls, p, docs, sep=b"\n"):
        stream, _ = stream_cases.join(docs, sep)
        code, d, tape, sbuf, table = many_device(p, Resident(p, stream))
        assert (code, d) == (0, len(docs)), (code, d)
        return cls(tape, sbuf, table)

    def parsed(self, d):
        """document d's own slices, as Python objects the model walks quickly"""
        t0, t1 = int(self.table["tape_begin"][d]), int(self.table["tape_begin"][d + 1])
        s0, s1 = int(self.table["string_begin"][d]), int(self.table["string_begin"][d + 1])
        return self.tape[t0:t1].tolist(), self.sbuf[s0:s1].tobytes(), t0, s0


def query(p, T, pointers, docs=None, raw=False, table_ptr=None, tape_ptr=None, value_skew=0):
    """-> (rc, tags[K, docs], values[K, docs]) from columns of exactly K * docs cells between poisoned guards"""
    torch = T.torch
    docs = T.docs if docs is None else docs
    K = len(pointers)
    cells = K * docs
    values = torch.full((cells + 2 * GUARD,), P64, dtype=torch.int64, device="cuda")
    tags = torch.full((cells + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = p.at_pointers_device(tape_ptr or T.d_tape.data_ptr(), len(T.tape), T.d_sbuf.data_ptr(), len(T.sbuf), table_ptr or T.d_table.data_ptr(), docs, pointers,
                              values.data_ptr() + 8 * GUARD + value_skew, tags.data_ptr() + GUARD, T.stream)
    torch.cuda.synchronize()
    vh, th = values.cpu().numpy().view(np.uint64), tags.cpu().numpy()
    written = cells if rc == 0 else 0
    assert (vh[:GUARD] == P64).all() and (vh[GUARD + written:] == P64).all(), "value poison"
    assert (th[:GUARD] == 0x5A).all() and (th[GUARD + written:] == 0x5A).all(), "tag poison"
    if raw:
        return rc
    assert rc == 0, (rc, p.last_error())
    return th[GUARD: GUARD + cells].reshape(K, docs).copy(), vh[GUARD: GUARD + cells].reshape(K, docs).copy()


def model(T, pointers, which=None):
    which = range(T.docs) if which is None else which
    tags, values = np.zeros((len(pointers), len(which)), np.uint8), np.zeros((len(pointers), len(which)), np.uint64)
    for j, d in enumerate(which):
        tape, sbuf, t0, s0 = T.parsed(d)
        for k, ptr in enumerate(pointers):
            tags[k, j], values[k, j] = pointer_model.walk(tape, sbuf, ptr, t0, s0)
    return tags, values


def assert_columns(got, want, what=""):
    for g, w, name in zip(got, want, ("tags", "values")):
        if not np.array_equal(g, w):
            k, d = np.argwhere(g != w)[0]
            raise AssertionError(f"{what}{name}[{k}, {d}] = {int(g[k, d])}, the model {int(w[k, d])}")


# ---- 1. the fixture -----------------------------------------------------------------------------------------------------------------------------
def test_fixture_as_one_stream_and_document_by_document(parser):
    import torch
    docs, pointers, cells = query_cases.fixture()
    T = Tapes.of_stream(parser, docs)
    for first in range(0, len(pointers), 64):
        tags, values = query(parser, T, pointers[first: first + 64])
        for i in range(len(docs)):
            for j in range(tags.shape[0]):
                assert query_cases.render(tags[j, i], values[j, i], T.sbuf) == cells[i][first + j], (docs[i][:80], pointers[first + j][:40])
        query_cases.check_container_cells(tags, values, T.tape, T.table)
    # every document alone through sjgpu_stage2_device, served by the table of two entries
    for i, d in enumerate(docs):
        res = Resident(parser, d)
        tape = torch.zeros(len(d) + 8, dtype=torch.int64, device="cuda")
        sbuf = torch.zeros(5 * (len(d) // 3) + 256, dtype=torch.uint8, device="cuda")
        rc, tw, sb = parser.stage2_device(res.buf.data_ptr(), res.length, res.idx.data_ptr(), res.n, tape.data_ptr(), len(d) + 8, sbuf.data_ptr(), sbuf.numel(), stream=res.stream)
        assert rc == 0
        table = np.zeros(2, capi.DOC_SPAN)
        table[1] = (res.n, len(d), tw, sb)
        one = Tapes(tape.cpu().numpy().view(np.uint64)[:tw], sbuf.cpu().numpy()[:sb], table)
        for first in range(0, len(pointers), 64):
            tags, values = query(parser, one, pointers[first: first + 64])
            for j in range(tags.shape[0]):
                assert query_cases.render(tags[j, 0], values[j, 0], one.sbuf) == cells[i][first + j], (d[:80], pointers[first + j][:40])


# ---- 2. random documents --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_tapes(parser):
    rng = np.random.default_rng(61)
    docs = stream_cases.valid_documents(rng, 2000)
    return docs, Tapes.of_stream(parser, docs)


def test_two_thousand_random_documents(parser, random_tapes):
    """32 pointers, 16 harvested from paths that exist in the documents and 16 that cannot hit; at least 30 % of the cells hits, at least 10 % each NO_SUCH_FIELD and
    INDEX_OUT_OF_BOUNDS, so that a run that finds nothing cannot pass.  These documents share no schema, so the harvest repeats the root pointer to get there
    (query_cases.harvest says how and why); the model alone, on the CPU: hits 32.1 %, NO_SUCH_FIELD 44.9 %, INDEX_OUT_OF_BOUNDS 17.2 %
    (tests/test_pointer_model.py::test_the_harvest_is_not_vacuous)."""
    docs, T = random_tapes
    pointers = query_cases.harvest(docs, 32)
    got, want = query(parser, T, pointers), model(T, pointers)
    assert_columns(got, want)
    query_cases.check_container_cells(got[0], got[1], T.tape, T.table)
    hits, nsf, oob = (got[0] >= 34).mean(), (got[0] == 20).mean(), (got[0] == 19).mean()
    print(f"hits {hits:.3f}, NO_SUCH_FIELD {nsf:.3f}, INDEX_OUT_OF_BOUNDS {oob:.3f}")
    assert hits >= 0.30 and nsf >= 0.10 and oob >= 0.10, (hits, nsf, oob)


def test_random_documents_distinct_paths(parser, random_tapes):
    """the same documents with the 16 commonest DISTINCT paths (second-level ones among them) and the 16 misses: cell for cell, no share asserted"""
    docs, T = random_tapes
    pointers = query_cases.distinct_harvest(docs, 32)
    assert len(set(pointers)) == 32
    got = query(parser, T, pointers)
    assert_columns(got, model(T, pointers))
    query_cases.check_container_cells(got[0], got[1], T.tape, T.table)
    assert (got[0] >= 34).sum() > 4000


# ---- 3. small records -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(parser):
    rng = np.random.default_rng(62)
    docs = stream_cases.small_records(rng, 200000)
    return docs, Tapes.of_stream(parser, docs)


def shape_of(doc):
    """what a small record's TAGS depend on: the record with its numbers and its filler text levelled"""
    return re.sub(rb"(lorem ipsum )+", b"L", re.sub(rb"\d+", b"0", doc))


def test_small_records(parser, small):
    docs, T = small
    pointers = query_cases.SMALL_RECORD_POINTERS
    tags, values = query(parser, T, pointers)
    # cell for cell against the model: the first blocks, every 16th document behind them and the last ones
    which = sorted(set(range(4200)) | set(range(4200, T.docs, 16)) | set(range(T.docs - 300, T.docs)))
    want = model(T, pointers, which)
    assert_columns((tags[:, which], values[:, which]), want)
    # every document's tags: a record's shape decides them, and there are few shapes
    by_shape = {}
    for d in which:
        by_shape.setdefault(shape_of(docs[d]), tags[:, d].tobytes())
    assert len(by_shape) < 40
    want_tags = np.frombuffer(b"".join(by_shape[shape_of(d)] for d in docs), np.uint8).reshape(T.docs, len(pointers)).T
    assert np.array_equal(tags, want_tags), np.argwhere(tags != want_tags)[:3]
    ids = np.array([k for k, d in enumerate(docs) if d.startswith(b'{"id":')])
    assert len(ids) > 30000 and np.array_equal(values[0, ids], ids.astype(np.uint64)) and (tags[0, ids] == ord("l")).all()  # "/id" of record k is k
    sample = np.zeros_like(tags)
    sample[:, which] = tags[:, which]
    query_cases.check_container_cells(sample, values, T.tape, T.table)
    assert (tags[9] >= 34).all() and (tags >= 34).mean() > 0.2


@pytest.mark.parametrize("docs", [1, 63, 64, 65, 257, 4097])
def test_small_records_in_front_of_a_cut(parser, small, docs):
    """odd rows, tag rows that begin at any byte, the edges of the launch blocks"""
    _, T = small
    pointers = query_cases.SMALL_RECORD_POINTERS
    got = query(parser, T, pointers, docs=docs)
    assert_columns(got, model(T, pointers, range(docs)))


# ---- 4. numbers that look like brackets -----------------------------------------------------------------------------------------------------------
def test_numbers_that_look_like_brackets(parser):
    docs = [b'[8863084066665136133,"x",{"k":1}]', b'[2.2181357552966544e+130,"x",{"k":2}]', b'{"n":8863084066665136133,"d":2.2181357552966544e+130,"k":"behind"}']
    T = Tapes.of_stream(parser, docs)
    assert int(T.tape[3]) == (ord("{") << 56) | 5 and int(T.tape[int(T.table["tape_begin"][1]) + 3]) >> 56 == ord("[")  # the value words the walk must not read as tags
    pointers = [b"/1", b"/2/k", b"/0", b"/k", b"/3"]
    tags, values = query(parser, T, pointers)
    assert_columns((tags, values), model(T, pointers))
    assert [chr(t) for t in tags[0, :2]] == ['"', '"'] and [pointer_model.string_of(T.sbuf, int(v)) for v in values[0, :2]] == [b"x", b"x"]
    assert [chr(t) for t in tags[1, :2]] == ["l", "l"] and values[1, :2].tolist() == [1, 2]
    assert chr(tags[3, 2]) == '"' and pointer_model.string_of(T.sbuf, int(values[3, 2])) == b"behind"
    assert values[2, 0] == 8863084066665136133 and tags[4, 0] == 19


# ---- 5. one long level ----------------------------------------------------------------------------------------------------------------------------
def test_one_long_level(parser):
    n = 20000
    obj = b"{" + b",".join(b'"key%d":{"v":{"w":[%d]},"s":"%d"}' % (i, i, i) for i in range(n)) + b"}"
    arr = b"[" + b",".join([b"%d" % i, b'"s%d"' % i, b"[[%d]]" % i, b'{"k":%d.5}' % i, b"null"][i % 5] for i in range(n)) + b"]"
    T = Tapes.of_stream(parser, [obj, arr])
    pointers = [b"/key0", b"/key19999", b"/key20000", b"/key1999", b"/key19999/v/w/0", b"/0", b"/19999", b"/20000", b"/19998/k", b""]
    tags, values = query(parser, T, pointers)
    assert_columns((tags, values), model(T, pointers))
    assert [chr(t) if t >= 34 else int(t) for t in tags[:, 0]] == ["{", "{", 20, "{", "l", 20, 20, 20, 20, "{"] and values[4, 0] == 19999
    assert [chr(t) if t >= 34 else int(t) for t in tags[:, 1]] == [17, 17, 17, 17, 17, "l", "n", 19, "d", "["]
    query_cases.check_container_cells(tags, values, T.tape, T.table)


# ---- 6. contract ----------------------------------------------------------------------------------------------------------------------------------
def test_contract(parser):
    import torch
    rng = np.random.default_rng(63)
    docs = stream_cases.small_records(rng, 300)
    T = Tapes.of_stream(parser, docs)
    pointers = [b"/id", b"/name", b"/0"]
    base = query(parser, T, pointers)
    assert query(parser, T, [], raw=True) == 0 and query(parser, T, pointers, docs=0, raw=True) == 0  # nothing written: the poison check inside
    assert query(parser, T, pointers, raw=True, tape_ptr=T.d_tape.data_ptr() + 4) == E_BADARG
    assert query(parser, T, pointers, raw=True, table_ptr=T.d_table.data_ptr() + 8) == E_BADARG
    assert query(parser, T, pointers, raw=True, value_skew=4) == E_BADARG
    assert query(parser, T, [b"/a"] * 65, raw=True) == E_BADARG and query(parser, T, [b"/a"] * 64, raw=True) == 0
    assert query(parser, T, [b"/" + b"a" * 1024], raw=True) == E_BADARG and query(parser, T, [b"/" + b"a" * 1023], raw=True) == 0
    assert query(parser, T, [b"/a" * 33], raw=True) == E_BADARG and query(parser, T, [b"/a" * 32], raw=True) == 0
    for field in ("tape_begin", "string_begin"):
        table = T.table.copy()
        table[field][[100, 101]] = table[field][[101, 100]]
        assert table[field][100] > table[field][101]
        back = torch.from_numpy(table.view(np.int32)).cuda()
        assert query(parser, T, pointers, raw=True, table_ptr=back.data_ptr()) == E_BADARG
    table = T.table.copy()
    table["tape_begin"][-1] += 1  # ends behind the tape
    assert query(parser, T, pointers, raw=True, table_ptr=torch.from_numpy(table.view(np.int32)).cuda().data_ptr()) == E_BADARG
    # a pointer without its leading slash is INVALID_JSON_POINTER for every document, and its neighbours' rows are what they were
    tags, values = query(parser, T, [b"id"] + pointers)
    assert (tags[0] == 22).all() and (values[0] == 0).all()
    assert_columns((tags[1:], values[1:]), base)
    assert parser.L.sjgpu_at_pointers_device(parser.h, None, 0, None, 0, None, 1, None, None, 0, None, None, None) == E_BADARG


# ---- 7. gather --------------------------------------------------------------------------------------------------------------------------------------
def gather(p, T, tags_row, values_row, chars_cap=None, want_total=None):
    """-> (rc, total, offsets[docs + 1], chars[total]) from outputs of exactly docs + 1 words and chars_cap bytes between poisoned guards"""
    torch = T.torch
    docs = len(tags_row)
    d_tags = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), tags_row])).cuda()  # the row begins at an odd address
    d_values = torch.from_numpy(np.ascontiguousarray(values_row).view(np.int64)).cuda() if docs else torch.zeros(1, dtype=torch.int64, device="cuda")
    chars_cap = want_total if chars_cap is None else chars_cap
    offsets = torch.full((docs + 1 + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    chars = torch.full((chars_cap + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    rc, total = p.gather_strings_device(T.d_sbuf.data_ptr(), len(T.sbuf), d_values.data_ptr(), d_tags.data_ptr() + 1, docs, offsets.data_ptr() + 4 * GUARD,
                                        chars.data_ptr() + GUARD, chars_cap, T.stream)
    oh, ch = offsets.cpu().numpy().view(np.uint32), chars.cpu().numpy()
    assert (oh[:GUARD] == 0x5A5A5A5A).all() and (oh[GUARD + docs + 1:] == 0x5A5A5A5A).all(), "offsets poison"
    written = total if rc == 0 else 0
    assert (ch[:GUARD] == 0x5A).all() and (ch[GUARD + written:] == 0x5A).all(), "character poison"
    return rc, total, oh[GUARD: GUARD + docs + 1].copy(), ch[GUARD: GUARD + written].tobytes()


def check_gather(p, T, tags_row, values_row, strings):
    lengths = np.array([len(s) for s in strings], np.uint64)
    total = int(lengths.sum())
    want_offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    rc, got_total, offsets, chars = gather(p, T, tags_row, values_row, want_total=total)  # exact capacity
    assert (rc, got_total) == (0, total) and np.array_equal(offsets, want_offsets) and chars == b"".join(strings)
    if total:
        rc, got_total, offsets, chars = gather(p, T, tags_row, values_row, chars_cap=total - 1)
        assert (rc, got_total, chars) == (E_OVERFLOW, total, b"") and np.array_equal(offsets, want_offsets)  # (... and the poison intact: checked inside)


def test_gather_columns_that_mix_everything(parser):
    big = np.random.default_rng(64).integers(0x20, 0x7F, 100 << 10, dtype=np.uint8).tobytes().replace(b'"', b"q").replace(b"\\", b"/")
    docs = []
    for k in range(5000):
        docs.append([b'{"s":"ab%d"}' % k, b'{"s":%d}' % k, b'{"t":"other"}', b'{"s":""}', b'{"s":"\\u00e9\\n%d","x":1}' % k, b'["s"]', b'{"s":null}'][k % 7])
    docs[2500] = b'{"x":[1,2],"s":"' + big + b'"}'
    T = Tapes.of_stream(parser, docs)
    pointers = [b"/s", b"/x", b"/0"]
    tags, values = query(parser, T, pointers)
    want = model(T, pointers)
    assert_columns((tags, values), want)
    strings = [pointer_model.string_of(T.sbuf, int(v)) if t == ord('"') else b"" for t, v in zip(want[0][0], want[1][0])]
    assert strings[2500] == big and strings[3] == b"" and sum(1 for s in strings if s) == 1 + sum(1 for k in range(5000) if k % 7 in (0, 4) and k != 2500)
    check_gather(parser, T, tags[0], values[0], strings)
    check_gather(parser, T, tags[1], values[1], [b""] * T.docs)  # no string at all: a total of 0
    check_gather(parser, T, tags[2], values[2], [b"s" if d == b'["s"]' else b"" for d in docs])
    rc, total, offsets, chars = gather(parser, T, tags[0][:0], values[0][:0], want_total=0)  # no documents
    assert (rc, total, offsets.tolist()) == (0, 0, [0])


def test_gather_two_columns_of_the_small_records(parser, small):
    docs, T = small
    pointers = [b"/name", b"/text"]
    tags, values = query(parser, T, pointers)
    for k, key in enumerate(("name", "text")):
        # the strings of every record from Python's json (the model is pinned against it on the CPU tier, and walks a sample here)
        strings = []
        for d in docs:
            v = json.loads(d) if d[:1] == b"{" else None
            s = v.get(key) if v else None
            strings.append(s.encode() if isinstance(s, str) else b"")
        which = range(0, T.docs, 97)
        mt, mv = model(T, pointers[k: k + 1], which)
        assert [pointer_model.string_of(T.sbuf, int(v)) if t == ord('"') else b"" for t, v in zip(mt[0], mv[0])] == [strings[d] for d in which]
        assert sum(1 for s in strings if s) > 30000
        check_gather(parser, T, tags[k], values[k], strings)


# ---- 8. extract_many --------------------------------------------------------------------------------------------------------------------------------
def test_extract_many_equals_the_device_entry_points(parser):
    rng = np.random.default_rng(65)
    pointers = [b"/id", b"/name", b"/tags/1", b"/0", b"", b"/a/b/c/1/d"]
    valid = stream_cases.small_records(rng, 3000)
    stream, _ = stream_cases.join(valid, b"\n")
    T = Tapes.of_stream(parser, valid)
    code, docs, tags, values = parser.extract_many(stream, pointers)
    assert (code, docs) == (0, 3000) and tags.shape == values.shape == (len(pointers), 3000)
    assert_columns((tags, values), query(parser, T, pointers))
    # a broken document in the middle: the documents in front of it, and its code
    broken = valid[:1200] + [b'{"a":tru}'] + valid[1200:]
    stream, _ = stream_cases.join(broken, b"\n")
    code, docs, tags, values = parser.extract_many(stream, pointers)
    assert (code, docs) == (6, 1200) and tags.shape == (len(pointers), 1200)
    assert_columns((tags, values), query(parser, T, pointers, docs=1200))
    assert parser.extract_many(b"", pointers)[:2] == (13, 0)
