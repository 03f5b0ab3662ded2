"""GPU tier (-m gpu): the entry point of include/sjgpu_json_wide.h on a caller's stream with inputs that arrive late -- the probe of tests/test_gpu_stream_order.py (its
world, side stream and delay, imported) over a case of its own, as tests/test_gpu_json_order.py has one for the narrow call.  The wide call waits for the stream three
times (the range space's size, the total, the fill), so its inputs must be real by the time it reads them; texts made from the decoy document are other texts."""
import numpy as np
import pytest

import json_text_model
import stream_order as so
from simdjson_amd import json_text_wide
from test_gpu_stream_order import delay, probe, roots_in, side, world  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def serialize_cells_wide_device(W):
    import torch
    X, p = W.twitter, W.parser()
    rows = len(W.users[0])
    rv, rt = roots_in(W.users)
    want = json_text_model.column(json_text_model.Stream(X.T.tape, X.T.sbuf, X.T.table), W.users)
    cap = len(want[1])
    assert cap > 10000 and not want[2].any()
    offsets, status, chars = so.poisoned(rows + 1, torch.int32), so.poisoned(rows, torch.uint8), so.poisoned(cap, torch.uint8)

    def enqueue(st):
        return json_text_wide.serialize_cells_wide_device(p, *X.args(), rv.ptr, rt.ptr, rows, offsets.data_ptr(), status.data_ptr(), chars.data_ptr(), cap, st)

    def check(ret, kept, note):
        assert ret == (0, cap), (ret, cap, note)
        assert np.array_equal(kept[1], want[2]), f"the statuses {note}"
        assert np.array_equal(kept[0], want[0]), f"the offsets {note}"
        assert kept[2].tobytes() == want[1], f"the texts {note}"
    return [so.Case("serialize_cells_wide_device", X.inputs + [rv, rt], [offsets, status, chars], enqueue, check)]


CASES = {"serialize_cells_wide_device": serialize_cells_wide_device}


@pytest.mark.parametrize("entry", list(CASES))
def test_entry_point_with_late_inputs(world, side, delay, entry):  # noqa: F811
    for case in CASES[entry](world):
        probe(case, side, delay)
