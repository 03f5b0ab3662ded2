"""GPU tier (-m gpu): the entry point of include/sjgpu_write.h on a caller's stream with inputs that arrive late -- the probe of tests/test_gpu_stream_order.py (its
world, side stream and delay, imported) over a case of its own, as tests/test_gpu_json_order.py has one.  It belongs in that module's TABLE, under the name of the
binding in simdjson_amd/writer.py, once it may be edited.  The call waits for the stream, so its inputs must be real by the time it reads them: every array of every
column is a late input -- the numbers over decoy_cells' words (every integer another one), the strings' characters over other letters, the validity words over
their complement --, and records made from the decoys are other records."""
import numpy as np
import pytest

import stream_order as so
import write_records_cases as cases
import write_records_model as model
from simdjson_amd import writer
from test_gpu_stream_order import delay, probe, side, world  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

N = 20000


def write_records_device(W):
    import torch
    p = W.parser()
    rng = np.random.default_rng(11)
    ints = rng.integers(0, 1 << 62, N).tolist()
    strings = [bytes(0x62 + (r + i) % 20 for i in range(r % 13)) for r in range(N)]  # letters b .. u: the decoy's are c .. v, no escape either way
    t = {"name": "late", "n": N, "columns": [cases.column(b"id", cases.INT64, [None if r % 5 == 0 else v for r, v in enumerate(ints)]),
                                             cases.column(b"name", cases.STRING, strings), cases.column(b"tag", cases.STRING_CELLS, strings[::-1])]}
    arrays = cases.arrays_of(t)
    want = model.records(arrays, cases.NEWLINE)
    cap = len(want[1])
    assert cap > 500000 and not want[2].any()
    late, columns = [], []
    for c in arrays["columns"]:
        d = {"key": c["key"], "kind": c["kind"], "chars_bytes": c["chars_bytes"]}
        if c["values"] is not None:  # (a string cell's word is where it lies: the same in the decoy)
            x = so.Late(c["values"], so.decoy_cells(c["values"]) if c["kind"] == cases.INT64 else None, pad=1)
            late.append(x)
            d["values"] = x.ptr
        if c["valid"] is not None:
            x = so.Late(c["valid"], ~c["valid"], pad=1)
            late.append(x)
            d["valid"] = x.ptr
        if c["offsets"] is not None:
            x = so.Late(c["offsets"], pad=1)
            late.append(x)
            d["offsets"] = x.ptr
        if c["chars"] is not None:
            x = so.Late(c["chars"], np.where(c["chars"] >= 0x62, c["chars"] + 1, c["chars"]).astype(np.uint8), pad=16)
            late.append(x)
            d["chars"] = x.ptr
        columns.append(d)
    offsets, status, chars, counts = so.poisoned(N + 1, torch.int32), so.poisoned(N, torch.uint8), so.poisoned(cap, torch.uint8), so.poisoned(4, torch.int64)

    def enqueue(st):
        return writer.write_records_device(p, columns, N, cases.NEWLINE, offsets.data_ptr(), status.data_ptr(), chars.data_ptr(), cap, counts.data_ptr(), st)

    def check(ret, kept, note):
        assert ret == (0, cap), (ret, cap, note)
        assert np.array_equal(kept[1], want[2]), f"the statuses {note}"
        assert np.array_equal(kept[0], want[0]), f"the offsets {note}"
        assert kept[2].tobytes() == want[1], f"the records {note}"
        assert np.array_equal(kept[3], want[3]), f"the counts {note}"
    return [so.Case("write_records_device", late, [offsets, status, chars, counts], enqueue, check)]


CASES = {"write_records_device": write_records_device}


@pytest.mark.parametrize("entry", list(CASES))
def test_entry_point_with_late_inputs(world, side, delay, entry):  # noqa: F811
    for case in CASES[entry](world):
        probe(case, side, delay)
