"""GPU tier (-m gpu): every call with u32 offsets and a 64-bit total at the limit of its offsets -- past 2^31 served, on 2^32 - 1 served, on 2^32 refused.

sjgpu_gather_strings_device, sjgpu_at_paths_device, sjgpu_at_paths_wide_device, sjgpu_at_paths_from_cells_device, sjgpu_object_fields_from_cells_device,
sjgpu_serialize_cells_device, sjgpu_write_records_device and sjgpu_write_nested_device count per cell, sum the counts into one 64-bit total, scan the counts in
place into u32 offsets (enqueue_scan, whose kernels work on int) and promise "A total beyond 32 bits: CAPACITY (1)".  The plan -- inputs, runs of rows, totals
-- is tests/offset_limit_cases.py; tests/test_offset_limit_cases.py (CPU tier) proves its sums by arithmetic and its row lengths by the Python models.  Nothing
expected here comes from the library: a total is rows x length, the offsets are an arithmetic progression, the bytes of a served column are ONE row of the model
broadcast over the rows.  The roots of the calls rooted at cells come from sjgpu_at_pointers_device and are compared with tests/pointer_model.py first.

Every output lies inside a larger tensor filled with 0x5A, 4 KiB of it on both sides (tests/test_gpu_exact_outputs.py's Out), and every comparison of a large
array runs on the device: no 2 GiB copy to the host.

    T1, count only   capacity 0 and null data pointers: SJGPU_E_OVERFLOW, the total exact, offsets[last] == total, all offsets the progression (uint32 widened to
                     int64), status and counts complete
    T1, served       the four calls that write bytes, at exactly T1 bytes of capacity: 0, every row the model's row -- the rows that end beyond 2^31 asserted by
                     themselves --, guards intact
    T2, count only   capacity 0 over a real, poisoned data buffer: SJGPU_E_OVERFLOW, total == offsets[last] == 0xFFFFFFFF, the progression, the poison intact
    T3               capacity 0 and capacity 1 MiB: CAPACITY, the true 64-bit total reported, status and counts complete, no byte of the data buffers written (a
                     wrapped total that "fits" 1 MiB would show as changed poison)

The calls that produce MATCHES or FIELDS are not filled at T1: 2^31 matches are 19 GiB of values and tags.  Their fill behind 2^31 stays unexercised."""
import time
import types

import numpy as np
import pytest

import json_text_model
import nested_write_model
import offset_limit_cases as C
import pointer_model
import write_records_model
from simdjson_amd import build, capi, json_text, writer
from test_gpu_exact_outputs import GUARD, POISON, Out
from test_gpu_query import Tapes, query

pytestmark = pytest.mark.gpu

E_OVERFLOW = capi.SJGPU_E_OVERFLOW
MIB = 1 << 20
CAP = 192 << 20


@pytest.fixture(scope="module")
def parser():
    build.build_sjgpu()
    p = capi.DomParserImplementation(CAP)
    yield p
    p.close()


@pytest.fixture(scope="module")
def env(parser):
    """what the cases read, resident: the document's own tapes (sjgpu_stage2_many_device) with the root cell of every pointer, the gather's string buffer with
    its three cells, the writers' characters"""
    import torch
    e = types.SimpleNamespace(p=parser, torch=torch)
    e.T = Tapes.of_stream(parser, [C.document()])
    names = list(C.ROOT_POINTERS)
    tags, values = query(parser, e.T, [C.ROOT_POINTERS[n] for n in names])
    tape, sbuf = e.T.tape.tolist(), e.T.sbuf.tobytes()
    e.cells = {}
    for k, n in enumerate(names):
        e.cells[n] = (int(tags[k, 0]), int(values[k, 0]))
        assert e.cells[n] == pointer_model.walk(tape, sbuf, C.ROOT_POINTERS[n]), n
    e.tape_args = (e.T.d_tape.data_ptr(), len(e.T.tape), e.T.d_sbuf.data_ptr(), len(e.T.sbuf), e.T.d_table.data_ptr(), e.T.docs)
    e.gather_sbuf_host, e.gather_cells = C.gather_buffer()
    e.gather_sbuf = torch.from_numpy(e.gather_sbuf_host).cuda()
    e.write_chars_host = C.write_chars()
    e.write_chars = torch.from_numpy(e.write_chars_host).cuda()
    e.stream = e.T.stream
    return e


# ---- rows and expectations on the device --------------------------------------------------------------------------------------------------------------------
def cells_of(e, case, cells):
    """the case's rows as root cells: (tags uint8[rows], values int64[rows]) of the device"""
    torch = e.torch
    tags = torch.cat([torch.full((count,), cells[name][0], dtype=torch.uint8, device="cuda") for name, count in case.runs])
    values = torch.cat([torch.full((count,), cells[name][1], dtype=torch.int64, device="cuda") for name, count in case.runs])
    return tags, values


def progression(e, lengths):
    """lengths: int64[...] of the host -> the offsets, int64[... + 1] of the device"""
    torch = e.torch
    d = torch.from_numpy(np.ascontiguousarray(lengths, np.int64)).cuda()
    return torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(d, 0)])


def widened(out):
    """an Out of u32 words -> int64 of the device, no value negative"""
    got = out.view(out.torch.int32).to(out.torch.int64) & 0xFFFFFFFF
    assert bool((got >= 0).all().item())
    return got


def fresh(torch, count, itemsize):
    out = Out(count, itemsize)
    out.torch = torch
    return out


class Call:
    """one call of a case: the offsets (and status, counts) between poisoned guards, the data arrays the caller hands in (None: null pointers)"""

    def __init__(self, e, rows, offsets_words, status_bytes, counts_words=0):
        t = e.torch
        self.e, self.rows = e, rows
        self.offsets = fresh(t, offsets_words, 4)
        self.status = fresh(t, status_bytes, 1) if status_bytes else None
        self.counts = fresh(t, counts_words, 8) if counts_words else None

    def check(self, what, rc, total, want_rc, want_total, lengths, data, written_bytes=None, counts=None):
        """rc and the total; offsets (unless the total wrapped them), status, counts; every guard; the data arrays untouched, or written up to written_bytes[i]"""
        assert (rc, total) == (want_rc, want_total), (what, rc, total, want_rc, want_total, self.e.p.last_error())
        assert self.offsets.intact_around(), (what, "poison around the offsets")
        if want_rc != capi.CAPACITY:  # (beyond 32 bits the offsets are written, and wrapped: they mean nothing)
            got = widened(self.offsets)
            assert int(got[-1].item()) == want_total, (what, "offsets[last]", int(got[-1].item()))
            want = progression(self.e, lengths)
            if not self.e.torch.equal(got, want):
                at = int((got != want).nonzero()[0].item())
                raise AssertionError(f"{what}: offsets[{at}] = {int(got[at].item())}, the progression has {int(want[at].item())}")
        if self.status is not None:
            assert self.status.intact_around() and not bool(self.status.view(self.e.torch.uint8).any().item()), (what, "a status that is not 0, or poison around the row")
        if self.counts is not None:
            assert self.counts.intact_around() and self.counts.view(self.e.torch.int64).tolist() == counts, (what, "counts", self.counts.view(self.e.torch.int64).tolist())
        for i, d in enumerate(data or ()):
            used = written_bytes[i] if written_bytes else 0
            assert d.intact_around(used), (what, f"data array {i}: poison changed outside its first {used} bytes")


def data_arrays(e, sizes, cap):
    """the data arrays of a call for `cap` entries of the given item sizes, poisoned"""
    return [fresh(e.torch, cap, size) for size in sizes]


def ptr(d, i):
    return d[i].ptr if d else 0


# ---- the eight calls, one shape: run(e, case, cap, data) -> (Call, rc, total, lengths, counts) ------------------------------------------------------------------
def run_gather(e, case, cap, data):
    tags, values = cells_of(e, case, e.gather_cells)
    rows = C.rows_of(case)
    c = Call(e, rows, rows + 1, 0)
    rc, total = e.p.gather_strings_device(e.gather_sbuf.data_ptr(), len(e.gather_sbuf_host), values.data_ptr(), tags.data_ptr(), rows, c.offsets.ptr, ptr(data, 0), cap, e.stream)
    e.torch.cuda.synchronize()
    return c, rc, total, C.lengths_of(case, C.GATHER_LENGTHS), None


def run_paths_from_cells(e, case, cap, data):
    tags, values = cells_of(e, case, e.cells)
    rows = C.rows_of(case)
    c = Call(e, rows, rows + 1, rows)
    rc, total = e.p.at_paths_from_cells_device(*e.tape_args, values.data_ptr(), tags.data_ptr(), rows, [C.PATH], c.offsets.ptr, c.status.ptr, ptr(data, 0), ptr(data, 1), cap, e.stream)
    e.torch.cuda.synchronize()
    return c, rc, total, C.lengths_of(case, C.PATH_LENGTHS), None


def run_fields_from_cells(e, case, cap, data):
    tags, values = cells_of(e, case, e.cells)
    rows = C.rows_of(case)
    c = Call(e, rows, rows + 1, rows)
    rc, total = e.p.object_fields_from_cells_device(*e.tape_args, values.data_ptr(), tags.data_ptr(), rows, c.offsets.ptr, c.status.ptr, ptr(data, 0), ptr(data, 1), ptr(data, 2),
                                                    ptr(data, 3), cap, e.stream)
    e.torch.cuda.synchronize()
    return c, rc, total, C.lengths_of(case, C.FIELD_LENGTHS), None


def run_serialize(e, case, cap, data):
    tags, values = cells_of(e, case, e.cells)
    rows = C.rows_of(case)
    c = Call(e, rows, rows + 1, rows)
    rc, total = json_text.serialize_cells_device(e.p, *e.tape_args, values.data_ptr(), tags.data_ptr(), rows, c.offsets.ptr, c.status.ptr, ptr(data, 0), cap, e.stream)
    e.torch.cuda.synchronize()
    return c, rc, total, C.lengths_of(case, C.TEXT_LENGTHS), None


def write_values(e, case, strings, elements=None):
    torch = e.torch
    return torch.cat([torch.full((count * (elements[name] if elements else 1),), C.string_cell(strings[name]), dtype=torch.int64, device="cuda") for name, count in case.runs])


def run_write_records(e, case, cap, data):
    values = write_values(e, case, C.WRITE_STRINGS)
    rows = C.rows_of(case)
    c = Call(e, rows, rows + 1, rows, 4)
    column = {"key": C.WRITE_KEY, "kind": capi.COL_STRING_CELLS, "values": values.data_ptr(), "chars": e.write_chars.data_ptr(), "chars_bytes": C.WRITE_CHARS}
    rc, total = writer.write_records_device(e.p, [column], rows, 0, c.offsets.ptr, c.status.ptr, ptr(data, 0), cap, c.counts.ptr, e.stream)
    e.torch.cuda.synchronize()
    return c, rc, total, C.lengths_of(case, C.WRITE_LENGTHS), [rows, 0, 0, 0]


def nested_field(e, case):
    """-> (the field of device addresses, what it points into, the elements)"""
    torch = e.torch
    values = write_values(e, case, C.NESTED_STRINGS, C.NESTED_ELEMENTS)
    per_row = np.concatenate([np.full(count, C.NESTED_ELEMENTS[name], np.int64) for name, count in case.runs])
    list_offsets = torch.from_numpy(np.concatenate([np.zeros(1, np.int64), np.cumsum(per_row)]).astype(np.int32)).cuda()
    field = {"key": C.WRITE_KEY, "kind": capi.COL_STRING_CELLS, "values": values.data_ptr(), "chars": e.write_chars.data_ptr(), "chars_bytes": C.WRITE_CHARS,
             "list_offsets": list_offsets.data_ptr(), "elements": values.numel()}
    return field, (values, list_offsets), int(values.numel())


def run_write_nested(e, case, cap, data):
    field, keep, elements = nested_field(e, case)
    rows = C.rows_of(case)
    c = Call(e, rows, rows + 1, rows, 6)
    rc, total = writer.write_nested_device(e.p, [field], rows, 0, c.offsets.ptr, c.status.ptr, ptr(data, 0), cap, c.counts.ptr, e.stream)
    e.torch.cuda.synchronize()
    del keep
    return c, rc, total, C.lengths_of(case, C.NESTED_LENGTHS), [rows, 0, 0, 0, elements, 0]


# call -> (its run, the item sizes of its data arrays)
CALLS = {"gather": (run_gather, (1,)), "paths_from_cells": (run_paths_from_cells, (8, 1)), "fields_from_cells": (run_fields_from_cells, (8, 1, 8, 1)),
         "serialize": (run_serialize, (1,)), "write_records": (run_write_records, (1,)), "write_nested": (run_write_nested, (1,))}
BYTE_WRITERS = ("gather", "serialize", "write_records", "write_nested")


def ids(cases):
    return [f"{c.call}: {c.name}" for c in cases]


def timed(what, t0):
    print(f"TIME {what}: {time.perf_counter() - t0:.2f} s")


def level(name):
    return [c for c in C.ALL_CASES if c.level == name]


# ---- T1 and T2: counted, not served -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", level("T1"), ids=ids(level("T1")))
def test_a_total_beyond_2_31_is_counted_exactly(env, case):
    """capacity 0, null data pointers: SJGPU_E_OVERFLOW with the total to allocate, every offset the progression"""
    t0 = time.perf_counter()
    run, _ = CALLS[case.call]
    c, rc, total, lengths, counts = run(env, case, 0, None)
    assert C.HALF < case.total < C.LIMIT
    c.check((case.call, case.name), rc, total, E_OVERFLOW, case.total, lengths, None, counts=counts)
    timed(f"{case.call} {case.name} counted", t0)


@pytest.mark.parametrize("case", level("T2"), ids=ids(level("T2")))
def test_a_total_of_2_32_minus_1_is_counted_exactly(env, case):
    """capacity 0 over real data arrays of 1 MiB entries: SJGPU_E_OVERFLOW, total == offsets[last] == 0xFFFFFFFF, the progression, the arrays' poison whole"""
    t0 = time.perf_counter()
    run, sizes = CALLS[case.call]
    data = data_arrays(env, sizes, MIB)
    c, rc, total, lengths, counts = run(env, case, 0, data)
    assert case.total == 0xFFFFFFFF
    c.check((case.call, case.name), rc, total, E_OVERFLOW, 0xFFFFFFFF, lengths, data, counts=counts)
    timed(f"{case.call} {case.name} counted", t0)


# ---- T1, served: the four calls that write bytes ---------------------------------------------------------------------------------------------------------------
def model_row(e, case):
    """the text of the case's one distinct row, from the Python models"""
    (name, _), = case.runs
    if case.call == "gather":
        return pointer_model.string_of(e.gather_sbuf_host, e.gather_cells[name][1])
    if case.call == "serialize":
        code, text = json_text_model.Stream(e.T.tape, e.T.sbuf, e.T.table).text_of(e.cells[name])
        assert code == 0
        return text
    if case.call == "write_records":
        return write_records_model.records(C.write_columns([name], e.write_chars_host), 0)[1]
    return nested_write_model.records(C.nested_fields([name], e.write_chars_host), 0)[1]


SERVED = [c for c in level("T1") if c.call in BYTE_WRITERS]


@pytest.mark.parametrize("case", SERVED, ids=ids(SERVED))
def test_a_column_beyond_2_31_bytes_is_served(env, case):
    """chars of exactly T1 bytes: rc 0, and chars[:T1] seen as rows x row_len is the model's row in every row -- the rows in front of 2^31 and the rows that end
    beyond it asserted one after the other, so a failure says which half broke"""
    torch = env.torch
    t0 = time.perf_counter()
    run, sizes = CALLS[case.call]
    rows, total = C.rows_of(case), case.total
    row = model_row(env, case)
    assert len(row) * rows == total
    data = data_arrays(env, sizes, total)
    c, rc, got_total, lengths, counts = run(env, case, total, data)
    c.check((case.call, case.name), rc, got_total, 0, total, lengths, data, written_bytes=[total], counts=counts)
    want = torch.from_numpy(np.frombuffer(row, np.uint8).copy()).cuda()
    same = (data[0].view(torch.uint8).view(rows, len(row)) == want).all(dim=1)  # per row, on the device
    first_beyond = C.HALF // len(row)  # the first row that ends beyond 2^31
    assert 0 < first_beyond < rows
    low, high = bool(same[:first_beyond].all().item()), bool(same[first_beyond:].all().item())
    bad = None if low and high else int((~same).nonzero()[0].item())
    del same, want, data, c
    torch.cuda.empty_cache()
    assert low, (case.call, case.name, "a row in front of 2^31 is not the model's", bad)
    assert high, (case.call, case.name, "a row that ends beyond 2^31 is not the model's", bad)
    timed(f"{case.call} {case.name} served", t0)


# ---- T3: refused ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, MIB], ids=["capacity 0", "capacity 1 MiB"])
@pytest.mark.parametrize("case", level("T3"), ids=ids(level("T3")))
def test_a_total_beyond_32_bits_is_refused(env, case, cap):
    """CAPACITY with the true 64-bit total, status and counts complete, and not a byte of the data arrays written: at 1 MiB of capacity a total that wrapped to
    0 (or to 65 536) would "fit" and the fill would run"""
    t0 = time.perf_counter()
    run, sizes = CALLS[case.call]
    data = data_arrays(env, sizes, MIB)
    c, rc, total, lengths, counts = run(env, case, cap, data)
    assert case.total >= C.LIMIT and (case.total & 0xFFFFFFFF) <= MIB
    c.check((case.call, case.name, cap), rc, total, capi.CAPACITY, case.total, lengths, data, counts=counts)
    timed(f"{case.call} {case.name} refused, capacity {cap}", t0)


@pytest.mark.parametrize("cap", [0, MIB], ids=["capacity 0", "capacity 1 MiB"])
def test_one_row_alone_beyond_32_bits_is_refused(env, cap):
    """sjgpu_write_records_device, n = 1, 64 columns of kind JSON over the same 64 MiB cell: the row's own u32 length wraps to 449, the 64-bit sum does not"""
    torch = env.torch
    t0 = time.perf_counter()
    chars = torch.full((C.WIDE_CELL,), ord("1"), dtype=torch.uint8, device="cuda")
    offsets = torch.tensor([0, C.WIDE_CELL], dtype=torch.int32, device="cuda")
    columns = [{"key": k, "kind": capi.COL_JSON, "offsets": offsets.data_ptr(), "chars": chars.data_ptr(), "chars_bytes": C.WIDE_CELL} for k in C.WIDE_KEYS]
    c = Call(env, 1, 2, 1, 4)
    data = data_arrays(env, (1,), MIB)
    rc, total = writer.write_records_device(env.p, columns, 1, 0, c.offsets.ptr, c.status.ptr, data[0].ptr, cap, c.counts.ptr, env.stream)
    torch.cuda.synchronize()
    assert C.WIDE_ROW_TOTAL == (1 << 32) + 449
    c.check("one row of 64 columns", rc, total, capi.CAPACITY, C.WIDE_ROW_TOTAL, None, data, counts=[1, 0, 0, 0])
    timed(f"write_records one row beyond 32 bits, capacity {cap}", t0)


# ---- the wrappers with a capacity retry ------------------------------------------------------------------------------------------------------------------------
def counting(monkeypatch, module, name):
    calls = []
    real = getattr(module, name)

    def counted(*args, **kwargs):
        out = real(*args, **kwargs)
        calls.append(out)
        return out
    monkeypatch.setattr(module, name, counted)
    return calls


def t3_of(call):
    return [c for c in C.ALL_CASES if c.call == call and c.name == "T3"][0]


def test_write_records_ends_with_capacity_after_one_call(env, monkeypatch):
    """writer.write_records over the T3 table: its first guess (2 MiB) is answered CAPACITY, which no larger array cures: ONE device call, and the SjgpuError it
    ends with carries the code"""
    case = t3_of("write_records")
    values = write_values(env, case, C.WRITE_STRINGS)
    calls = counting(monkeypatch, writer, "write_records_device")
    with pytest.raises(capi.SjgpuError) as caught:
        writer.write_records(env.p, [{"key": C.WRITE_KEY, "kind": capi.COL_STRING_CELLS, "values": values, "chars": env.write_chars}], C.rows_of(case), newline=False)
    assert calls == [(capi.CAPACITY, case.total)] and caught.value.code == capi.CAPACITY


def test_write_nested_ends_with_capacity_after_one_call(env, monkeypatch):
    torch = env.torch
    case = t3_of("write_nested")
    rows = C.rows_of(case)
    values = write_values(env, case, C.NESTED_STRINGS)
    list_offsets = torch.arange(rows + 1, dtype=torch.int32, device="cuda")
    calls = counting(monkeypatch, writer, "write_nested_device")
    with pytest.raises(capi.SjgpuError) as caught:
        writer.write_nested(env.p, [{"key": C.WRITE_KEY, "kind": capi.COL_STRING_CELLS, "values": values, "chars": env.write_chars, "list_offsets": list_offsets, "elements": rows}],
                            rows, newline=False)
    assert calls == [(capi.CAPACITY, case.total)] and caught.value.code == capi.CAPACITY


def test_the_json_column_call_returns_capacity_after_one_call(env, monkeypatch):
    """json_text's call behind capi._to_capacity, as json_column_many makes it: (CAPACITY, the total, ...) from ONE device call"""
    torch = env.torch
    case = t3_of("serialize")
    rows = C.rows_of(case)
    tags, values = cells_of(env, case, env.cells)
    S = types.SimpleNamespace(dev=torch.device("cuda", env.p.device), stream=env.stream, args=lambda: env.tape_args)
    offsets = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
    status = torch.empty(rows, dtype=torch.uint8, device="cuda")
    calls = counting(monkeypatch, json_text, "serialize_cells_device")
    roots = (values.data_ptr(), tags.data_ptr(), rows)
    rc, needed, chars = capi._to_capacity(lambda cap: json_text._serialize(env.p, S, roots, offsets, status, cap), MIB)
    assert (rc, needed) == (capi.CAPACITY, case.total) and calls == [(capi.CAPACITY, case.total)] and chars.numel() == MIB


# ---- the calls rooted at documents: sjgpu_at_paths_device and sjgpu_at_paths_wide_device ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def streams(parser):
    """the two streams of arrays of ones, resident with their tapes: made when a case first asks, one at a time (each is ~136 MB of text and ~2 GB of tapes)"""
    import torch
    held = {}

    def get(name):
        if name not in held:
            held.clear()
            torch.cuda.empty_cache()
            elements = C.STREAMS[name]
            S = capi.ResidentStream(parser, C.roots_stream(elements), doc_cap=len(elements) + 1)
            assert (S.code, S.docs) == (0, len(elements)), (S.code, S.docs)
            held[name] = S
        return held[name]
    yield get
    held.clear()
    torch.cuda.empty_cache()


ROOT_CALLS = ("at_paths_device", "at_paths_wide_device")


@pytest.mark.parametrize("wide", [False, True], ids=["depth first", "wide"])
@pytest.mark.parametrize("case", C.ROOTS, ids=[c.name for c in C.ROOTS])
def test_paths_rooted_at_documents_at_the_limit(env, streams, case, wide):
    """T1 and T2 with capacity 0 (T1: null data pointers; T2: real arrays, their poison whole): SJGPU_E_OVERFLOW, the total exact, the offsets -- path k, document d
    at k * docs + d -- the progression; T3 with capacity 0 and with 1 MiB: CAPACITY, 2^32 reported, nothing written"""
    t0 = time.perf_counter()
    S = streams(case.stream)
    call = getattr(env.p, ROOT_CALLS[wide])
    K, docs = len(case.paths), S.docs
    lengths = C.roots_lengths(case)
    for cap in ((0, MIB) if case.level == "T3" else (0,)):
        data = None if case.level == "T1" else data_arrays(env, (8, 1), MIB)
        c = Call(env, K * docs, K * docs + 1, K * docs)
        rc, total = call(*S.args(), list(case.paths), c.offsets.ptr, c.status.ptr, ptr(data, 0), ptr(data, 1), cap, S.stream)
        env.torch.cuda.synchronize()
        c.check((ROOT_CALLS[wide], case.name, cap), rc, total, capi.CAPACITY if case.level == "T3" else E_OVERFLOW, case.total, lengths, data)
    timed(f"{ROOT_CALLS[wide]} {case.name}", t0)
