"""GPU tier (-m gpu): the entry point of include/sjgpu_nested.h on a caller's stream with inputs that arrive late -- the probe of tests/test_gpu_stream_order.py (its
world, side stream and delay, imported) over a case of its own, as tests/test_gpu_write_order.py has one.  The call waits for the stream, so its inputs must be real
by the time it reads them: every array of every field is a late input -- the elements over decoy_cells' words, the strings' characters over other letters, the
validity words (the elements' and the lists') over their complement, the list offsets over zeros --, and rows made from the decoys are other rows."""
import numpy as np
import pytest

import nested_write_cases as cases
import nested_write_model as model
import stream_order as so
from simdjson_amd import writer
from test_gpu_stream_order import delay, probe, side, world  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

N = 20000


def write_nested_device(W):
    import torch
    p = W.parser()
    rng = np.random.default_rng(12)
    ints = rng.integers(0, 1 << 62, 3 * N).tolist()
    strings = [bytes(0x62 + (r + i) % 20 for i in range(r % 13)) for r in range(N)]  # letters b .. u: the decoy's are c .. v, no escape either way
    t = {"name": "late", "n": N, "fields": [cases.list_field(b"ids", cases.INT64, [None if r % 7 == 0 else [None if (r + i) % 5 == 0 else ints[3 * r + i] for i in range(r % 4)] for r in range(N)]),
                                            cases.list_field(b"names", cases.STRING, [[strings[r], strings[N - 1 - r]][: r % 3] for r in range(N)]),
                                            cases.column(b"tag", cases.STRING_CELLS, strings[::-1])]}
    arrays = cases.arrays_of(t, lead=2)
    want = model.records(arrays, cases.NEWLINE)
    cap = len(want[1])
    assert cap > 500000 and not want[2].any()
    late, fields = [], []
    for f in arrays["fields"]:
        d = {"key": f["key"], "kind": f["kind"], "chars_bytes": f["chars_bytes"], "elements": f["elements"]}
        if f["values"] is not None:  # (a string cell's word is where it lies: the same in the decoy)
            x = so.Late(f["values"], so.decoy_cells(f["values"]) if f["kind"] == cases.INT64 else None, pad=1)
            late.append(x)
            d["values"] = x.ptr
        for name in ("valid", "list_valid"):
            if f[name] is not None:
                x = so.Late(f[name], ~f[name], pad=1)
                late.append(x)
                d[name] = x.ptr
        if f["offsets"] is not None:
            x = so.Late(f["offsets"], pad=1)
            late.append(x)
            d["offsets"] = x.ptr
        if f["list_offsets"] is not None:
            x = so.Late(f["list_offsets"], np.zeros_like(f["list_offsets"]), pad=1)
            late.append(x)
            d["list_offsets"] = x.ptr
        if f["chars"] is not None:
            x = so.Late(f["chars"], np.where(f["chars"] >= 0x62, f["chars"] + 1, f["chars"]).astype(np.uint8), pad=16)
            late.append(x)
            d["chars"] = x.ptr
        fields.append(d)
    offsets, status, chars, counts = so.poisoned(N + 1, torch.int32), so.poisoned(N, torch.uint8), so.poisoned(cap, torch.uint8), so.poisoned(6, torch.int64)

    def enqueue(st):
        return writer.write_nested_device(p, fields, N, cases.NEWLINE, offsets.data_ptr(), status.data_ptr(), chars.data_ptr(), cap, counts.data_ptr(), st)

    def check(ret, kept, note):
        assert ret == (0, cap), (ret, cap, note)
        assert np.array_equal(kept[1], want[2]), f"the statuses {note}"
        assert np.array_equal(kept[0], want[0]), f"the offsets {note}"
        assert kept[2].tobytes() == want[1], f"the rows {note}"
        assert np.array_equal(kept[3], want[3]), f"the counts {note}"
    return [so.Case("write_nested_device", late, [offsets, status, chars, counts], enqueue, check)]


CASES = {"write_nested_device": write_nested_device}


@pytest.mark.parametrize("entry", list(CASES))
def test_entry_point_with_late_inputs(world, side, delay, entry):  # noqa: F811
    for case in CASES[entry](world):
        probe(case, side, delay)
